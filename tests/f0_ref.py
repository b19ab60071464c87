"""Yardstick of the YIN pitch tracker (test infrastructure, never imported by the product): the definition of include/psnd.h written out
frame by frame in float64, from the definition and not from `kernels.yin_f0_host` (which runs over all frames at once, lag by lag; here one
frame at a time, all lags of it at once, the decisions of steps 3-5 as plain Python loops).

Besides (f0, aperiodicity, lag) every frame gets a MARGIN: how far, relative to the threshold, the nearest of its decisions was from going
the other way - the smallest of
    (d'(tau) - thr) / thr   over the lags of the search range in front of t0 (over the whole range on an unvoiced frame),
    (thr - d'(t0)) / thr,
    |d'(t + 1) - d'(t)| / thr   for every comparison the descent makes, the one that stops it included.
A frame decided by rule 6 (a non-finite sample) has margin inf: no arithmetic is involved.  An implementation in other arithmetic must
choose the same lag wherever the margin exceeds its rounding.

`dtype=np.float32, reverse=True` is the same definition in float32 with the sum over j taken from the last term to the first: "the same
arithmetic in another order", its f0 and aperiodicity rounded to float32 as an output in that precision is.  Tolerances of the GPU tests
are taken from that variant's distance to float64, never from the kernel."""
import math

import numpy as np


def lags(sr, f0_floor=71.0, f0_ceil=800.0, frame_length=None):
    tau_min = max(2, int(math.floor(sr / f0_ceil)))
    tau_max = int(math.ceil(sr / f0_floor))
    return tau_min, tau_max, (2 * tau_max if frame_length is None else int(frame_length))


def frames(T, hop):
    return T // hop + 1


def frame(x, i, hop, sr, tau_min, tau_max, W, thr, dtype=np.float64, reverse=False):
    """frame i of the row x -> (f0, aperiodicity, lag, margin)"""
    T, span = len(x), W + tau_max
    lo = i * hop - span // 2
    u = np.zeros(span, dtype=dtype)
    a, b = max(lo, 0), min(lo + span, T)
    if b > a:
        u[a - lo:b - lo] = x[a:b]
    if not np.isfinite(u).all():
        return 0.0, 1.0, 0, math.inf
    e = u[:W][None, :] - np.lib.stride_tricks.sliding_window_view(u, W)[1:tau_max + 1]       # row tau - 1: u[j] - u[j + tau]
    sq = e * e
    if dtype == np.float64:
        d = sq.sum(axis=1)
    else:                                               # a running sum in the working precision, in the order asked for
        d = np.cumsum(sq[:, ::-1] if reverse else sq, axis=1, dtype=dtype)[:, -1]
    dp = np.ones(tau_max + 1, dtype=dtype)
    run = dtype(0)
    for tau in range(1, tau_max + 1):
        run = dtype(run + d[tau - 1])
        dp[tau] = dtype(1) if run == 0 else dtype(dtype(d[tau - 1] * dtype(tau)) / run)
    thr = dtype(thr)
    margins, t0 = [], 0
    for tau in range(tau_min, tau_max + 1):
        if dp[tau] < thr:
            t0 = tau
            break
        margins.append((float(dp[tau]) - float(thr)) / float(thr))
    if t0 == 0:
        return 0.0, float(dp[tau_min:].min()), 0, min(margins)          # dp is of the working precision: so is what is returned
    margins.append((float(thr) - float(dp[t0])) / float(thr))
    t = t0
    while t + 1 <= tau_max:
        margins.append(abs(float(dp[t + 1]) - float(dp[t])) / float(thr))
        if not dp[t + 1] < dp[t]:
            break
        t += 1
    off = dtype(0)
    if t - 1 >= 1 and t + 1 <= tau_max:
        y0, y1, y2 = dp[t - 1], dp[t], dp[t + 1]
        den = dtype(dtype(y0 - dtype(2) * y1) + y2)
        if den > 0:
            off = min(max(dtype(dtype(0.5) * dtype(y0 - y2)) / den, dtype(-0.5)), dtype(0.5))
    return float(dtype(float(sr) / (float(t) + float(off)))), float(dp[t]), t, min(margins)       # f0 rounded as the output would be


def track(x, hop, sr, tau_min, tau_max, W, thr, dtype=np.float64, reverse=False):
    """every frame of one row -> (f0 float64 (F,), aperiodicity float64 (F,), lag int32 (F,), margin float64 (F,))"""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    F = frames(len(x), hop)
    out = [frame(x, i, hop, sr, tau_min, tau_max, W, thr, dtype, reverse) for i in range(F)]
    return (np.array([o[0] for o in out], dtype=np.float64), np.array([o[1] for o in out], dtype=np.float64),
            np.array([o[2] for o in out], dtype=np.int32), np.array([o[3] for o in out], dtype=np.float64))


def get_f0(x, hop, sr=22050, f0_floor=71.0, f0_ceil=800.0, threshold=0.1, frame_length=None, **kw):
    """the public function's arguments -> track(...)"""
    tau_min, tau_max, W = lags(sr, f0_floor, f0_ceil, frame_length)
    return track(x, hop, sr, tau_min, tau_max, W, threshold, **kw)


def spans_with(sample, T, hop, span):
    """the frames whose span [i hop - span // 2, i hop - span // 2 + span) holds the sample index `sample`"""
    return [i for i in range(frames(T, hop)) if i * hop - span // 2 <= sample < i * hop - span // 2 + span]


def glide(sr, T, sigma=0.0, seed=0, quiet=None):
    """the input family of the GPU tests: three harmonics (1, 0.8, 0.6) of a fundamental gliding linearly from 140 Hz to 224 Hz over the row,
    3 Hz amplitude modulation of depth 0.3, peak about 0.9; white noise of deviation `sigma` on top; `quiet` = (a, b): the samples [a, b)
    scaled by 1e-3 (YIN is scale-free: a quiet stretch must track like a loud one).  float32."""
    t = np.arange(T) / float(sr)
    f = 140.0 + (224.0 - 140.0) * np.arange(T) / max(T - 1, 1)
    ph = 2.0 * np.pi * np.cumsum(f) / float(sr)
    x = (np.sin(ph) + 0.8 * np.sin(2.0 * ph + 0.7) + 0.6 * np.sin(3.0 * ph + 1.9)) / 2.4
    x *= 0.9 * (1.0 - 0.3 * (0.5 + 0.5 * np.sin(2.0 * np.pi * 3.0 * t)))
    if sigma:
        x = x + np.random.RandomState(1000 + seed).randn(T) * sigma
    if quiet:
        x[quiet[0]:quiet[1]] *= 1e-3
    return x.astype(np.float32)


# the four configurations the definition was prototyped on: (sr, hop, T, f0_floor) - tau_max 311 (no multiple of 64), 256 (a multiple),
# 40 with tau_min 10 (less than one wave of lags), and a hop beyond the span
CONFIGS = ((22050, 32, 8000, 71.0), (16000, 1, 700, 62.5), (8000, 50, 3000, 200.0), (22050, 2000, 9000, 71.0))
# one more of this file's own: hop 1 on a row longer than the span (the 700 samples of the second are shorter than its span of 768, so
# all its frames reach over an end and none is voiced) - tau_max 80, W 160, 3001 frames
EXTRA = ((8000, 1, 3000, 100.0),)
SIGMAS = (0.0, 0.05, 0.1, 0.2)
KEEP = 1e-3                 # frames with a margin of at least this are compared lag for lag
LEFT_OUT = 0.03             # at most this fraction of a case's frames may fall under KEEP
