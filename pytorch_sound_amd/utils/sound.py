"""pytorch_sound/utils/sound.py: the filters, on numpy arrays as the reference has them and on tensors of either device.

    preemphasis, inv_preemphasis   the reference's two scipy.signal.lfilter calls (:66-71)
    lowpass, highpass, biquad      two-pole sections (the reference's lowpass pipes the array through sox, :25-35)
    get_wav_duration               :52-63
    resample                       sample-rate conversion (the reference shells out: scripts/preprocess.py:82-88 sox, :32-41 ffmpeg)

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


def get_wav_duration(file):
    """duration of a wave file in seconds, -1 where it cannot be read (sound.py:52-63)"""
    try:
        sr, wav = wav_read(file)
        return len(wav) / sr
    except Exception:      # noqa: BLE001 - the reference swallows everything here
        return -1
