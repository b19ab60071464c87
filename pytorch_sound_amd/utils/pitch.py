"""Fundamental frequency per frame, on numpy arrays and on tensors of either device: what stands in this project where the reference's
`utils/sound.py` has `get_f0` (:38-49).

    get_f0(wav, hop_length, sr=22050, ...)                 f0 in Hz per frame, 0.0 where the frame is unvoiced, float32
    get_f0_with_confidence(wav, hop_length, sr=22050, ...) (f0, aperiodicity): the value of d' at the chosen lag, small = periodic

NOT the reference's estimator.  There `get_f0` calls WORLD's DIO and StoneMask through `pyworld`, a package this project does not depend on
and cannot run, so its output can neither be recorded nor pinned: parity with WORLD DIO + StoneMask is UNPINNED, as `lowpass` is against
sox and `resample` against sox / ffmpeg (`utils/sound.py`).  What is implemented is one published, fully specified estimator, YIN
(A. de Cheveigne, H. Kawahara, "YIN, a fundamental frequency estimator for speech and music", JASA 111 (4), 2002), steps 1-5, by the
definition written out in include/psnd.h.  Kept of the reference's contract: the argument names (wav, hop_length, sr=22050), one value per
frame at the times i hop_length / sr, T // hop_length + 1 frames (WORLD's frame count for frame_period = 1000 hop_length / sr, taken as
exact integer arithmetic), 0.0 for an unvoiced frame, float32 out, WORLD's default search range of 71-800 Hz, and no padding (the
reference's `pad_center(wav, len(wav))` pads nothing).

The definition.  tau_min = max(2, floor(sr / f0_ceil)), tau_max = ceil(sr / f0_floor), W = frame_length or 2 tau_max (W >= tau_max),
span = W + tau_max, H = span // 2.  Frame i reads u[j] = wav[i hop_length - H + j], j < span, with zeros outside the signal:

    1  d(tau) = sum_{j < W} (u[j] - u[j + tau])^2 for tau = 1 .. tau_max
    2  d'(tau) = d(tau) tau / sum_{k <= tau} d(k), and 1 where that sum is 0
    3  t0 = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold; none: the frame is unvoiced, aperiodicity = min d'
    4  t = t0, and on to t + 1 while d'(t + 1) < d'(t) and t + 1 <= tau_max
    5  f0 = sr / (t + off), off in [-1/2, 1/2] the vertex of the parabola through d'(t - 1), d'(t), d'(t + 1) where both neighbours
       exist and the parabola opens upwards, else 0; aperiodicity = d'(t)
    6  a frame whose span holds a NaN or an Inf is unvoiced with aperiodicity 1, and such a sample touches no other frame

Frames whose span reaches over an end of the signal see zeros there: the first and last H / hop_length frames compare signal with silence
and tend to come out unvoiced.  The output is not differentiable (a lag is an integer; f0 jumps where it changes).

A numpy array or a CPU tensor goes through the float64 restatement `kernels.yin_f0_host`; a HIP tensor (float32; float16 / bfloat16 are
cast, float64 raises) through the one launch of psnd_pitch.hip (`kernels.yin_f0`) with no host synchronisation and no copy.  A 1-D input is
one row, leading axes are batch: (..., T) in, (..., T // hop_length + 1) out.  `lengths` (one integer per row) marks a zero-padded batch as
ragged rows: row n has lengths[n] // hop_length + 1 frames, whatever lies behind its length is read as zeros, its other slots are 0.

Not here: pYIN / Viterbi smoothing, a gradient, streaming use.
"""
import numpy as np

from .. import kernels


def _run(wav, hop_length, sr, f0_floor, f0_ceil, threshold, frame_length, lengths):
    import torch
    if isinstance(wav, torch.Tensor):
        f0, ap, _ = kernels.yin_f0(wav, hop_length, sr, f0_floor, f0_ceil, threshold, frame_length, lengths)
        return f0, ap
    x = np.asarray(wav)
    if not np.issubdtype(x.dtype, np.floating):
        x = x.astype(np.float64)
    f0, ap, _ = kernels.yin_f0(torch.from_numpy(np.ascontiguousarray(x)), hop_length, sr, f0_floor, f0_ceil, threshold, frame_length, lengths)
    return f0.numpy(), ap.numpy()


def get_f0(wav, hop_length, sr=22050, f0_floor=71.0, f0_ceil=800.0, threshold=0.1, frame_length=None, lengths=None):
    """f0 in Hz at the samples 0, hop_length, 2 hop_length, ...: (..., T // hop_length + 1) float32, 0.0 where unvoiced.  YIN by the
    definition in the module docstring; parity with the reference's WORLD DIO + StoneMask is unpinned."""
    return _run(wav, hop_length, sr, f0_floor, f0_ceil, threshold, frame_length, lengths)[0]


def get_f0_with_confidence(wav, hop_length, sr=22050, f0_floor=71.0, f0_ceil=800.0, threshold=0.1, frame_length=None, lengths=None):
    """(f0, aperiodicity), both (..., T // hop_length + 1) float32: aperiodicity is d' at the chosen lag (below `threshold` on a voiced
    frame), the smallest d' of the search range on an unvoiced one, 1 where the frame holds a non-finite sample or lies behind its row"""
    return _run(wav, hop_length, sr, f0_floor, f0_ceil, threshold, frame_length, lengths)
