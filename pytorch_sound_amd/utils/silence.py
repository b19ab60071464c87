"""pytorch_sound/utils/silence.py: pydub's silence detector on sample arrays, as the reference has it on numpy and here on tensors of either
device as well.

    rms, db_to_float                     plain arithmetic (:9-22)
    detect_silence, detect_nonsilent     lists of [start, end] sample ranges (:25-107)
    split_on_silence                     the non-silent stretches as slices of the input (:110-135; scripts/preprocess.py:109-137 cuts long
                                         recordings into clips with it)

Lengths are counts of SAMPLES, though the reference's parameter names say "ms".  The definition is the one of include/psnd.h: windows of
`min_silence_len` samples start at 0, seek_step, 2 seek_step, ... and at the last possible place; a window is silent iff its energy
sum x^2 <= min_silence_len 10^(silence_thresh / 10) - the reference's rms <= 10^(silence_thresh / 20) - and it holds no NaN or Inf; silent
starts merge into ranges in order.  A 1-D numpy array or CPU tensor goes through the vectorised host restatement of `kernels` (float64
energies from block-local prefix sums); a HIP tensor through the three launches of psnd_silence.hip (`kernels.silence_ranges`) and ONE
device-to-host copy, of the ranges - the audio stays where it is, and the chunks of `split_on_silence` are views of it.  A 2-D tensor or
array (N, T), with optional per-row `lengths` for a zero-padded batch, gives one list per row from one call of the kernels.

Not covered: energies are float64 sums of float32 samples, the reference's are float32 dot products, so a window whose rms equals the
threshold to within float32 rounding may be decided the other way (the golden cases keep a margin of 1e-3 and agree exactly); a
window's energy is resolved to 2^-52 of the energy of the 1024-sample blocks it touches, so at -inf dB samples below about 1e-8 of their
loud neighbours in the same block count as zeros; integer sample arrays are read as their float64 values, where the reference's dot
product wraps around; a per-sample silence mask and pydub's AudioSegment front end are not here, nor is the reference's
`parse_midi` helper of another module (pitch per frame: `utils.pitch`).
"""
import numpy as np

from .. import kernels


def _is_tensor(x):
    import torch
    return isinstance(x, torch.Tensor)


def rms(x):
    """sqrt(mean x^2) of a 1-D array (:9-10); of a tensor, a 0-dim tensor on its device"""
    if _is_tensor(x):
        return (x.dot(x) / x.numel()).sqrt()
    return np.sqrt(x.dot(x) / x.size)


def db_to_float(db, using_amplitude=True):
    """a level in dB as a ratio of amplitudes (10^(db / 20)) or of powers (10^(db / 10))"""
    return 10 ** (float(db) / (20 if using_amplitude else 10))


def _row_lengths(x, lengths):
    N, T = x.shape
    if lengths is None:
        return [T] * N
    lens = lengths.tolist() if hasattr(lengths, 'tolist') else list(lengths)
    if len(lens) != N:
        raise ValueError('silence: %d lengths for %d rows' % (len(lens), N))
    return [min(max(int(v), 0), T) for v in lens]


def _silent(x, min_silence_len, silence_thresh, seek_step, lengths):
    """-> (the input is a batch, per-row silent ranges, per-row lengths); a 1-D input is one row"""
    if x.ndim not in (1, 2):
        raise ValueError('silence: a 1-D signal or a 2-D batch (N, T) is expected, got shape %s' % (tuple(x.shape),))
    if x.ndim == 1 and lengths is not None:
        raise ValueError('silence: lengths go with a 2-D batch')
    lens = [x.shape[0]] if x.ndim == 1 else _row_lengths(x, lengths)
    if _is_tensor(x):
        _, ranges = kernels.silence_ranges(x, min_silence_len, silence_thresh, seek_step, None if x.ndim == 1 else lengths)
        ranges = ranges.cpu().numpy()                   # the one copy; the -1 fill marks each row's end
        out = [r[r[:, 0] >= 0].tolist() for r in ranges]
    else:
        L, s = kernels.silence_params(min_silence_len, seek_step)
        theta = kernels.silence_theta(L, silence_thresh)
        rows = [x] if x.ndim == 1 else [x[n, :lens[n]] for n in range(x.shape[0])]
        out = [kernels.silence_ranges_host(r, L, s, theta).tolist() for r in rows]
    return x.ndim == 2, out, lens


def _nonsilent(silent, length):
    """the gaps between the silent ranges of a row of `length` samples (:83-107)"""
    if not silent:
        return [[0, length]]
    if silent[0] == [0, length]:
        return []
    starts = [0] + [e for _, e in silent]
    ends = [b for b, _ in silent] + [length]
    out = [[a, b] for a, b in zip(starts, ends)]
    if out[-1][0] == length:                            # the last silence runs to the end
        out.pop()
    if out[0] == [0, 0]:                                # the first one starts the row
        out.pop(0)
    return out


def detect_silence(audio_segment, min_silence_len=1000, silence_thresh=-16, seek_step=1, lengths=None):
    """[[start, end], ...] of the silent stretches at least `min_silence_len` samples long; for a batch (N, T) one such list per row"""
    x = audio_segment if _is_tensor(audio_segment) else np.asarray(audio_segment)
    batch, silent, _ = _silent(x, min_silence_len, silence_thresh, seek_step, lengths)
    return silent if batch else silent[0]


def detect_nonsilent(audio_segment, min_silence_len=1000, silence_thresh=-16, seek_step=1, lengths=None):
    """[[start, end], ...] of what lies between the silent stretches; the whole signal where there is none, [] where all is silent"""
    x = audio_segment if _is_tensor(audio_segment) else np.asarray(audio_segment)
    batch, silent, lens = _silent(x, min_silence_len, silence_thresh, seek_step, lengths)
    out = [_nonsilent(r, n) for r, n in zip(silent, lens)]
    return out if batch else out[0]


def split_on_silence(audio_segment, min_silence_len=1000, silence_thresh=-16, keep_silence=100, seek_step=1, lengths=None):
    """the non-silent stretches, each widened by `keep_silence` samples on both sides (the end un-clamped, as the reference slices), as
    slices of the input: views for an array or a tensor.  For a batch (N, T) one list per row, sliced from the row's valid part."""
    x = audio_segment if _is_tensor(audio_segment) else np.asarray(audio_segment)
    batch, silent, lens = _silent(x, min_silence_len, silence_thresh, seek_step, lengths)
    out = []
    for n, (r, length) in enumerate(zip(silent, lens)):
        row = x[n, :length] if batch else x
        out.append([row[max(0, a - keep_silence):b + keep_silence] for a, b in _nonsilent(r, length)])
    return out if batch else out[0]
