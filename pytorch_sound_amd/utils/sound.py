"""pytorch_sound/utils/sound.py: the filters, on numpy arrays as the reference has them and on tensors of either device.

    preemphasis, inv_preemphasis   the reference's two scipy.signal.lfilter calls (:66-71)
    lowpass, highpass, biquad      two-pole sections (the reference's lowpass pipes the array through sox, :25-35)
    get_wav_duration               :52-63
    resample                       sample-rate conversion (the reference shells out: scripts/preprocess.py:82-88 sox, :32-41 ffmpeg)
    time_stretch, pitch_shift      duration without pitch and pitch without duration (the reference reaches sox's `tempo` / `pitch` through
                                   pysndfx's AudioEffectsChain)
    griffinlim                     a waveform from a magnitude spectrogram alone (the reference has none; it imports librosa throughout)
    mel_to_magnitude, mel_to_wave  a linear magnitude, and a waveform, from a mel spectrogram alone (the reference has none)
    loudness, normalize            integrated loudness in LUFS and level normalisation (the reference runs every file through
                                   ffmpeg-normalize on the host: scripts/preprocess.py:32-41)
    add_noise                      a signal with noise mixed in at a wanted SNR (torchaudio's add_noise; the reference's
                                   make_background_numpy only cuts the noise beds: scripts/preprocess.py)

A numpy array goes through scipy on the host, exactly as in the reference.  A torch tensor comes back as a tensor of the same dtype and
device through `kernels.lfilter`: on a HIP tensor the native scan of psnd_lfilter.hip in both directions (differentiable in the signal,
no host round trip, no library op), on a CPU tensor scipy in float64.  All filters run along the last axis with zero initial state.

Not here: `parse_midi` (pretty_midi) and `get_f0` (pyworld, librosa) - host-only wrappers around packages this project does not depend on.
A pitch tracker of this project's own - YIN, not WORLD, so under another roof - is `utils.pitch.get_f0`, with the reference's arguments.

`lowpass` is NOT pinned against the reference: its output there is whatever the installed sox computes (through pysndfx), which this
project cannot run.  What is implemented is the two-pole low-pass of the Audio EQ Cookbook, the design sox documents for its `lowpass`
effect, in floating point without sox's clipping at full scale; the tests check it by known answers (DC gain, -3 dB at the cutoff),
not against sox output.  The defaults (44.1 kHz, q = 0.707) are pysndfx's as remembered, not verified.

`resample` is NOT pinned against the reference either, for the same reason: there the rate is changed by `sox ... rate` or by ffmpeg, whose
filters this project can neither run nor read off.  What is implemented is scipy.signal.resample_poly, on which the reference already
depends through scipy: with up / down = new_sr / orig_sr in lowest terms and P = 10 max(up, down), the linear-phase low-pass
firwin(2P + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up applied between zero-stuffing by `up` and keeping every `down`-th sample,
zeros beyond both ends, ceil(T up / down) samples out.  A numpy array goes through scipy itself; a HIP tensor through the polyphase kernel of
psnd_resample.hip (`kernels.resample_poly`), which is that sum in float32 and whose gradient is the same kernel the other way round.

`time_stretch` and `pitch_shift` are NOT pinned against the reference either: parity with sox's `tempo` and `pitch` is UNPINNED.  sox
changes the time scale by WSOLA (overlap-add of waveform segments picked by correlation); what is implemented here is the plain phase
vocoder of torchaudio's `phase_vocoder` and librosa's `time_stretch` / `pitch_shift`, by the definition written out in include/psnd.h:
STFT, output frame j at the input time j rate with an interpolated magnitude and an accumulated phase advance, inverse STFT; the pitch
shift is that stretch followed by `resample_poly` with the fraction `kernels.pitch_ratio` picks.  On a HIP tensor all three steps are
native (`STFT.transform_complex`, psnd_phase_vocoder.hip, `psnd_istft_reim`; the phase is summed as a fixed-point fraction of a turn, so
a long clip keeps it); numpy arrays and CPU tensors run the same definition in float64 numpy between the host STFTs.  No transient or
formant handling, no phase locking, no gradient.

`griffinlim` is not something the reference has, so there is no parity to pin: it is torchaudio's `functional.griffinlim` / librosa's
`griffinlim` (fast Griffin-Lim, Perraudin et al. 2013) by the definition written out in include/psnd.h, on this project's `STFT` - the
reference's framing and inverse (`transform_complex`, `inverse_complex`), not torch.stft's.  On a HIP tensor every iteration is the two
native transforms and one launch of psnd_griffinlim.hip between them; numpy arrays and CPU tensors run the same loop in float64 through
the host transforms.  No early stopping, no gradient.

`mel_to_magnitude` is the mel-inverse section of include/psnd.h: per frame the non-negative least-squares problem of the row-normalised
filterbank, a fixed number of FISTA steps from a flat-band guess - one launch of psnd_mel_inverse.hip on a HIP tensor, float64 numpy on
numpy arrays and CPU tensors.  torchaudio's `InverseMelScale` and librosa's `mel_to_stft` are other algorithms: parity unpinned.
`mel_to_wave` is `mel_to_magnitude` followed by `griffinlim`.  No gradient.

`loudness` and `normalize` are NOT pinned against the reference either: parity with ffmpeg-normalize's numbers is UNPINNED, because this
project cannot run ffmpeg.  What is implemented is the loudness section of include/psnd.h: ITU-R BS.1770-4 / EBU R128 integrated loudness
(K-weighting re-derived for the rate at hand, blocks of 400 ms every 100 ms, the absolute gate at -70 LUFS and the relative gate 10 LU
below the ungated mean), and for kind 'rms' / 'peak' the plain level 10 log10(mean x^2) / 20 log10(max |x|) - 'rms' is the mode
`process_all` asks ffmpeg-normalize for.  No oversampled true peak, no short-term loudness, no loudness range, no limiter: a gain only.
On a HIP tensor the meter is psnd_loudness.hip (one read of every sample per launch, the filtered signal never written) and the gain is
applied from device memory: no host round trip, a call can be captured; numpy arrays and CPU tensors run the same definition in float64
numpy.  The tests check known answers (a 997 Hz sine at 0 dBFS reads -3.01 LUFS) and a sequential yardstick.  No gradient.
"""
import math

import numpy as np
from scipy import signal
from scipy.io.wavfile import read as wav_read

from .. import kernels


def _is_tensor(x):
    import torch
    return isinstance(x, torch.Tensor)


def biquad(x, b, a):
    """one filter section of order <= 2 along the last axis, zero initial state: scipy.signal.lfilter(b, a, x).  numpy in -> float32 numpy
    out (as the reference's filters); tensor in -> tensor of the same dtype and device out."""
    if _is_tensor(x):
        return kernels.lfilter(x, b, a)
    kernels.lfilter_section(b, a)                       # the same argument checks on both paths
    return signal.lfilter(b, a, x).astype(np.float32)


def preemphasis(x, coeff=0.97):
    """y[t] = x[t] - coeff x[t-1] with x[-1] = 0 (sound.py:66-67).  `models.sound.PreEmphasis` reflect-pads one sample instead (x[-1] = x[1]):
    the two differ in sample 0 only."""
    return biquad(x, [1, -coeff], [1])


def inv_preemphasis(x, coeff=0.97):
    """y[t] = x[t] + coeff y[t-1] with y[-1] = 0 (sound.py:70-71): the exact inverse of `preemphasis`.  (`models.sound.InversePreEmphasis`
    is the reference's tanh RNN, not this filter.)"""
    return biquad(x, [1], [1, -coeff])


def _cookbook(frequency, sample_rate, q):
    w0 = 2.0 * math.pi * float(frequency) / float(sample_rate)
    return math.cos(w0), math.sin(w0) / (2.0 * float(q))


def lowpass_coefficients(frequency, sample_rate=44100, q=0.707):
    """(b, a) of the Audio EQ Cookbook two-pole low-pass: w0 = 2 pi f / fs, alpha = sin w0 / (2 q)"""
    c, alpha = _cookbook(frequency, sample_rate, q)
    return [(1 - c) / 2, 1 - c, (1 - c) / 2], [1 + alpha, -2 * c, 1 - alpha]


def highpass_coefficients(frequency, sample_rate=44100, q=0.707):
    """(b, a) of the cookbook two-pole high-pass, the mirror image of the low-pass"""
    c, alpha = _cookbook(frequency, sample_rate, q)
    return [(1 + c) / 2, -(1 + c), (1 + c) / 2], [1 + alpha, -2 * c, 1 - alpha]


def lowpass(wav, frequency, sample_rate=44100, q=0.707):
    """two-pole low-pass at `frequency` Hz (sound.py:25-35).  Parity with the reference's sox output is unpinned: module docstring."""
    return biquad(wav, *lowpass_coefficients(frequency, sample_rate, q))


def highpass(wav, frequency, sample_rate=44100, q=0.707):
    """two-pole high-pass at `frequency` Hz; not in the reference, the counterpart of `lowpass`"""
    return biquad(wav, *highpass_coefficients(frequency, sample_rate, q))


def resample(wav, orig_sr, new_sr):
    """`wav` at orig_sr Hz converted to new_sr Hz along the last axis (integer rates): scipy.signal.resample_poly's definition, module
    docstring.  numpy in -> float32 numpy out; tensor in -> tensor of the same dtype and device out.  Equal rates return a copy.  Not pinned
    against the reference's sox / ffmpeg output."""
    up, down = kernels.resample_ratio(orig_sr, new_sr)
    if _is_tensor(wav):
        return kernels.resample_poly(wav, up, down)
    wav = np.asarray(wav)
    if wav.ndim == 0:
        raise kernels.PsndError('resample: the input needs a time axis')
    if up == down:
        return wav.astype(np.float32)                   # a copy, as scipy's
    if wav.size == 0:
        return np.zeros(wav.shape[:-1] + (-(-wav.shape[-1] * up // down),), dtype=np.float32)
    return signal.resample_poly(wav.astype(np.float64), up, down, axis=-1).astype(np.float32)


_STFTS = {}


def _stft(n_fft, hop_length):
    """one STFT module per (n_fft, hop_length): its plans are cached per device, so a later call copies nothing from the host"""
    from ..models.transforms import STFT
    key = (int(n_fft), int(hop_length))
    if key not in _STFTS:
        if key[0] < 2 or key[1] < 1:
            raise ValueError('time_stretch: n_fft=%r hop_length=%r' % (n_fft, hop_length))
        _STFTS[key] = STFT(key[0], key[1])
    return _STFTS[key]


def _fix_length(y, n):
    """the last axis trimmed or zero-padded to n samples"""
    import torch
    if y.shape[-1] >= n:
        return y[..., :n].contiguous()
    return torch.nn.functional.pad(y, (0, n - y.shape[-1]))


def _effect(fn, wav, what):
    """numpy in -> float32 numpy out through the CPU path; tensor in -> tensor of the same dtype and device out, no graph.  fn takes and
    returns (N, T) rows in float32 (float64 stays float64 on the CPU; on a HIP tensor it raises)."""
    import torch
    if not _is_tensor(wav):
        x = np.asarray(wav)
        if x.ndim == 0:
            raise kernels.PsndError('%s: the input needs a time axis' % what)
        return _effect(fn, torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), what).numpy()
    if wav.dim() == 0:
        raise kernels.PsndError('%s: the input needs a time axis' % what)
    if not wav.is_floating_point():
        raise kernels.PsndError('%s: floating input expected, got %s' % (what, wav.dtype))
    if wav.is_cuda and wav.dtype == torch.float64:
        raise kernels.PsndError('%s: no float64 instance on HIP tensors: pass a float32 tensor, or a CPU tensor in float64' % what)
    with torch.no_grad():
        rows = wav.detach().reshape(-1, wav.shape[-1])
        y = fn(rows if rows.dtype == torch.float64 else rows.float())
    return y.to(wav.dtype).reshape(wav.shape[:-1] + (y.shape[-1],))


def stretch_rows(rows, rate, stft):
    """(N, T) -> (N, round(T / rate)): stft.transform_complex, kernels.phase_vocoder, stft.inverse_complex, trimmed or zero-padded"""
    re, im = stft.transform_complex(rows)
    yr, yi = kernels.phase_vocoder(re, im, rate)
    return _fix_length(stft.inverse_complex(yr, yi), int(round(rows.shape[-1] / rate)))


def shift_rows(rows, ratio, stft, device_taps=None):
    """(N, T) -> (N, T): stretched by q / p, then resampled by q / p, for ratio = (p, q) = kernels.pitch_ratio(...)"""
    p, q = ratio
    y = stretch_rows(rows, q / p, stft)
    return _fix_length(kernels.resample_poly(y, q, p, device_taps=device_taps), rows.shape[-1])


def time_stretch(wav, rate, n_fft=1024, hop_length=256):
    """`wav` (..., T) made 1 / rate times as long without changing its pitch (rate > 1: faster and shorter), int(round(T / rate))
    samples out (librosa's rule): STFT(n_fft, hop_length).transform_complex, kernels.phase_vocoder, inverse_complex.  The plain phase
    vocoder of torchaudio / librosa, no transient handling; not sox's `tempo` (WSOLA) - module docstring.  T must exceed n_fft / 2
    (the transform's reflect padding).  numpy in -> float32 numpy out; tensor in -> tensor of the same dtype and device out.  No gradient."""
    rate = kernels._pv_rate(rate)
    stft = _stft(n_fft, hop_length)
    return _effect(lambda rows: stretch_rows(rows, rate, stft), wav, 'time_stretch')


def pitch_shift(wav, sr, n_steps, bins_per_octave=12, n_fft=1024, hop_length=256):
    """`wav` (..., T) shifted by `n_steps` steps of an octave / `bins_per_octave` at unchanged length T (librosa's arguments; `sr` does not
    enter): with (p, q) = kernels.pitch_ratio(n_steps, bins_per_octave), resample_poly(time_stretch(wav, q / p), up=q, down=p), trimmed or
    zero-padded to T.  The interval is the fraction p / q (max(p, q) <= 640, within 0.03 cent of the semitones up to an octave), not the
    irrational 2 ** (n_steps / bins_per_octave).  Not sox's `pitch` - module docstring.  numpy in -> float32 numpy out; tensor in ->
    tensor of the same dtype and device out.  No gradient."""
    if not float(sr) > 0.0:
        raise ValueError('pitch_shift: sr=%r must be positive' % (sr,))
    ratio = kernels.pitch_ratio(n_steps, bins_per_octave)
    stft = _stft(n_fft, hop_length)
    return _effect(lambda rows: shift_rows(rows, ratio, stft), wav, 'pitch_shift')


def griffinlim(magnitude, n_iter=32, n_fft=None, hop_length=None, momentum=0.99, length=None, init_phase=None, rand_init=True):
    """a waveform (..., length or (F - 1) hop_length) whose STFT magnitude approaches `magnitude` (..., K, F): `n_iter` iterations of fast
    Griffin-Lim (torchaudio's / librosa's definition, include/psnd.h) with momentum in [0, 1) on STFT(n_fft, hop_length) of this project;
    n_fft defaults to 2 (K - 1), hop_length to n_fft // 4.  `init_phase` (the magnitude's shape) sets the first phase, else `rand_init`
    draws it uniformly once, else it is 0.  `kernels.griffinlim` does the work.  numpy in -> float32 numpy out; tensor in -> tensor of the
    same dtype and device out (float64 on a HIP tensor raises).  No gradient."""
    import torch
    if not _is_tensor(magnitude):
        m = np.asarray(magnitude)
        if m.ndim < 2:
            raise kernels.PsndError('griffinlim: the input needs a bin and a frame axis')
        if init_phase is not None:
            init_phase = torch.from_numpy(np.ascontiguousarray(init_phase, dtype=np.float32))
        return griffinlim(torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32)), n_iter, n_fft, hop_length, momentum, length, init_phase,
                          rand_init).numpy()
    if magnitude.dim() < 2:
        raise kernels.PsndError('griffinlim: the input needs a bin and a frame axis')
    if n_fft is None:
        n_fft = 2 * (magnitude.shape[-2] - 1)
    if hop_length is None:
        hop_length = n_fft // 4
    return kernels.griffinlim(magnitude, _stft(n_fft, hop_length), n_iter, momentum, length, init_phase, rand_init)


_LOG_KINDS = {None: kernels.LOG_NONE, 'e': kernels.LOG_E, 'ln': kernels.LOG_E, 'log': kernels.LOG_E, '10': kernels.LOG_10,
              'log10': kernels.LOG_10}


def _log_kind(log):
    try:
        return _LOG_KINDS[log]
    except (KeyError, TypeError):
        raise ValueError("log=%r - None (a linear mel), 'e' or '10'" % (log,))


def _mel_plan(mel_filter, n_iter):
    """a `kernels.MelInversePlan` as it is, a filterbank as a plan built for this call (nothing is cached on a tensor's address: a caller
    with many calls builds the plan once with `kernels.mel_inverse_plan` and passes it, or uses `InverseMelScale` / `MelToWave`)"""
    if isinstance(mel_filter, kernels.MelInversePlan):
        return mel_filter
    return kernels.mel_inverse_plan(mel_filter, max(n_iter, kernels.MEL_INVERSE_ITER_MAX))


def mel_to_magnitude(mel, mel_filter, n_iter=64, log=None, log_offset=1e-6, frames=None, return_residual=False):
    """a linear magnitude (..., K, F) >= 0 whose projection by `mel_filter` (M, K), finite and >= 0, approaches the mel spectrogram `mel`
    (..., M, F): `kernels.mel_inverse`, `n_iter` FISTA steps per frame by the definition of include/psnd.h.  `log`: None for a linear mel,
    'e' for log(lin + log_offset) (what LogMelSpectrogram gives), '10' for log10(lin + log_offset); `log_offset` is ignored for a linear
    mel.  `mel_filter` may be a `kernels.MelInversePlan` (`kernels.mel_inverse_plan(mel_filter)`): the filterbank itself costs a plan
    built on the host and copied to the device in every call, the plan nothing after its first use.  numpy in -> float32 numpy out; tensor in -> tensor of the same dtype and device
    out (float64 on a HIP tensor raises).  No gradient."""
    import torch
    kind = _log_kind(log)
    off = float(log_offset) if kind != kernels.LOG_NONE else 0.0
    if not _is_tensor(mel):
        m = np.ascontiguousarray(np.asarray(mel), dtype=np.float32)
        r = mel_to_magnitude(torch.from_numpy(m), mel_filter, n_iter, log, log_offset, frames, return_residual)
        return (r[0].numpy(), r[1].numpy().astype(np.float32)) if return_residual else r.numpy()
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
        raise ValueError('mel_to_magnitude: n_iter=%r - an integer >= 0' % (n_iter,))
    return kernels.mel_inverse(mel, _mel_plan(mel_filter, n_iter), n_iter, kind, off, frames, return_residual)


def mel_to_wave(mel, mel_filter, n_fft=None, hop_length=None, n_iter=64, gl_iter=32, momentum=0.99, log=None, log_offset=1e-6, length=None,
                rand_init=True):
    """a waveform (..., length or (F - 1) hop_length) from a mel spectrogram (..., M, F) alone: `mel_to_magnitude` (`n_iter` steps), then
    `griffinlim` (`gl_iter` iterations, `momentum`) on STFT(n_fft, hop_length) of this project; n_fft defaults to 2 (K - 1), hop_length to
    n_fft // 4.  Two calls of the library's loops on a HIP tensor, nothing leaves the device.  No gradient."""
    mag = mel_to_magnitude(mel, mel_filter, n_iter, log, log_offset)
    return griffinlim(mag, gl_iter, n_fft, hop_length, momentum, length, None, rand_init)


def loudness(wav, sr, lengths=None, channels=None, weights=None, return_blocks=False):
    """integrated loudness in LUFS of every programme of `wav` at `sr` Hz (ITU-R BS.1770-4 / EBU R128, include/psnd.h): float32 of the
    leading shape, numpy in -> numpy out, tensor in -> tensor on the same device out.  `wav` is (..., T), every row a mono programme, or
    (..., C, T) with channels=C (weights default to 1, 1, 1, 1.41, 1.41).  -inf: silent or shorter than 400 ms; NaN: a non-finite sample.
    `kernels.loudness` does the work.  Parity with ffmpeg's ebur128 is unpinned: module docstring."""
    return kernels.loudness(wav, sr, lengths, channels, weights, return_blocks)


NORMALIZE_KINDS = ('ebu', 'rms', 'peak')


def normalize(wav, sr, target_level=-23.0, kind='ebu', lengths=None, channels=None):
    """`wav` with every programme scaled by one gain so that it measures `target_level`: LUFS for kind 'ebu' (`loudness`), dB re full
    scale of its rms for 'rms' and of its sample peak for 'peak' (`sr` enters for 'ebu' only).  A programme whose level is not finite -
    silent, shorter than a block of 400 ms ('ebu'), holding a non-finite sample - comes back unchanged; samples behind `lengths` are
    copied.  No limiter: the result may exceed full scale.  numpy in -> float32 numpy out; tensor in -> tensor of the same dtype and
    device out; on a HIP tensor two native calls (the meter, then the gain read from device memory), no host round trip, capturable.
    No gradient (a tensor that requires grad comes back detached, as from `time_stretch`).  Parity with ffmpeg-normalize is unpinned:
    module docstring."""
    import torch
    if kind not in NORMALIZE_KINDS:
        raise ValueError("normalize: kind=%r - 'ebu', 'rms' or 'peak'" % (kind,))
    target = float(target_level)
    if not math.isfinite(target):
        raise ValueError('normalize: target_level=%r' % (target_level,))
    if _is_tensor(wav) and wav.is_cuda:
        with torch.no_grad():
            if kind == 'ebu':
                gain = kernels.loudness_gain(wav, sr, target, lengths, channels)[1]
            else:
                gain = kernels.level_gain(wav, kind, target, lengths, channels)[1]
            return kernels.apply_gain(wav, gain, lengths, channels)
    if _is_tensor(wav):
        if not wav.is_floating_point():
            raise kernels.PsndError('normalize: floating input expected, got %s' % wav.dtype)
        x = wav.detach().to(torch.float64).numpy()
    else:
        x = np.asarray(wav)
    level = kernels.loudness_host(x, sr, lengths, channels) if kind == 'ebu' else kernels.level_host(x, kind, lengths, channels)
    y = kernels.apply_gain_host(x, kernels.gain_of_level(level, target), lengths, channels)
    return torch.from_numpy(y).to(wav.dtype) if _is_tensor(wav) else y


def add_noise(wav, noise, snr, lengths=None):
    """`wav` with `noise` mixed in at `snr` dB per row of (..., T), torchaudio's `add_noise` by the definition of include/psnd.h:
    wav + g noise before a row's length and wav behind it, g = sqrt(sum wav^2 / sum noise^2) 10^(-snr / 20) from float64 sums.  `snr`: one
    number or one per row.  A row that is silent in either input, or holds a non-finite sample, comes back unchanged.  numpy in ->
    float32 numpy out; tensor in -> tensor of the same dtype and device out; on HIP tensors `kernels.mix_at_snr` (psnd_separation.hip),
    the gain never leaves the device and the call can be captured.  Not differentiable: an input that requires grad raises."""
    for v in (wav, noise, snr):
        if _is_tensor(v) and v.requires_grad:
            raise kernels.PsndError('add_noise is not differentiable: detach the inputs')
    if _is_tensor(wav) != _is_tensor(noise):
        raise kernels.PsndError('add_noise: signal and noise must both be tensors or both be arrays')
    return kernels.mix_at_snr(wav, noise, snr, lengths)


def get_wav_duration(file):
    """duration of a wave file in seconds, -1 where it cannot be read (sound.py:52-63)"""
    try:
        sr, wav = wav_read(file)
        return len(wav) / sr
    except Exception:      # noqa: BLE001 - the reference swallows everything here
        return -1
