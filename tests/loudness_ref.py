"""Yardstick of the loudness tests: ITU-R BS.1770-4 / EBU R128 integrated loudness as plain sequential Python and numpy in float64 (test
infrastructure, imports nothing of pytorch_sound_amd).  The definition is the loudness section of include/psnd.h.

`measure(x, sr)` takes ONE programme, (T,) or (C, T), and returns a `Reading`: lufs (a Python float: -inf, or NaN for a programme with a
non-finite sample), z (the block energies, float64) and margin, the smallest relative distance of any z[j] from either gate - a test input
must keep it above MARGIN, so that no rounding of the code under test can move a block across a gate.
"""
import collections
import math

import numpy as np

MARGIN = 1e-6
GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)

Reading = collections.namedtuple('Reading', 'lufs z margin')


def k_weighting(sr):
    """[(b, a) of the shelf, (b, a) of the high-pass], a[0] = 1"""
    out = []
    for f0, Q, shelf in ((1681.974450955533, 0.7071752369554196, True), (38.13547087602444, 0.5003270373238773, False)):
        K = math.tan(math.pi * f0 / sr)
        a0 = 1.0 + K / Q + K * K
        a = [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
        if shelf:
            Vh = 10.0 ** (3.999843853973347 / 20.0)
            Vb = Vh ** 0.4996667741545416
            b = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
        else:
            b = [1.0, -2.0, 1.0]
        out.append((b, a))
    return out


def block(sr):
    B = int(math.floor(0.4 * sr + 0.5))
    return B, B // 4


def n_blocks(T, B, H):
    return 0 if T < B else (T - B) // H + 1


def biquad(b, a, x):
    """one section, zero state before t = 0, sample after sample in Python floats (float64)"""
    b0, b1, b2 = b
    _, a1, a2 = a
    y = [0.0] * len(x)
    x1 = x2 = y1 = y2 = 0.0
    for t, v in enumerate(x):
        w = b0 * v + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1, y2, y1 = x1, v, y1, w
        y[t] = w
    return y


def gates(z):
    """(lufs, margin) of block energies z"""
    if len(z) == 0:
        return -math.inf, math.inf
    margin = float(np.min(np.abs(z / GATE - 1.0)))
    za = z[z > GATE]
    if za.size == 0:
        return -math.inf, margin
    gamma = 0.1 * float(np.mean(za))
    margin = min(margin, float(np.min(np.abs(z / gamma - 1.0))))
    zg = za[za > gamma]
    return -0.691 + 10.0 * math.log10(float(np.mean(zg))), margin


def measure(x, sr, weights=None):
    x = np.asarray(x)
    x = x[None] if x.ndim == 1 else x
    C, T = x.shape
    G = WEIGHTS[:C] if weights is None else tuple(float(w) for w in weights)
    assert len(G) == C
    B, H = block(sr)
    J = n_blocks(T, B, H)
    if not np.isfinite(x).all():
        return Reading(math.nan, np.full(J, np.nan), math.inf)
    z = np.zeros(J, dtype=np.float64)
    if J:
        (b1, a1), (b2, a2) = k_weighting(sr)
        for c in range(C):
            y = np.asarray(biquad(b2, a2, biquad(b1, a1, x[c].astype(np.float64).tolist())), dtype=np.float64)
            y2 = y * y
            z += G[c] * np.asarray([float(np.sum(y2[j * H:j * H + B])) for j in range(J)]) / B
    lufs, margin = gates(z)
    return Reading(lufs, z, margin)


def rms_db(x):
    x = np.asarray(x, dtype=np.float64)
    return 10.0 * math.log10(float(np.mean(x * x))) if x.size and np.any(x) else -math.inf


def peak_db(x):
    x = np.asarray(x, dtype=np.float64)
    return 20.0 * math.log10(float(np.max(np.abs(x)))) if x.size and np.any(x) else -math.inf


# ---- the inputs both test files use -------------------------------------------------------------------------------------------------------
def gated_noise(seed, T, sr, C=None):
    """noise whose gain changes every 0.3 s over 60 dB (steps of 6 dB, shuffled), with one stretch of 0.9 s far below the absolute gate
    where there are six stretches or more, so both gates cut blocks: float32 (T,) or (C, T)"""
    g = np.random.RandomState(seed)
    shape = (T,) if C is None else (C, T)
    n = g.standard_normal(shape)
    seg = max(1, int(0.3 * sr))
    k = -(-T // seg)
    db = -6.0 * (g.permutation(k) % 11)
    if k >= 6:
        at = g.randint(k - 2)
        db[at:at + 3] = -90.0
    env = np.repeat(10.0 ** (db / 20.0), seg)[:T]
    return (0.25 * n * env).astype(np.float32)


def two_level_sine(sr=16000, seconds=3.0, drop_db=30.0, freq=440.0, amp=0.5):
    n = int(seconds * sr)
    t = np.arange(2 * n) / sr
    x = amp * np.sin(2.0 * math.pi * freq * t)
    x[n:] *= 10.0 ** (-drop_db / 20.0)
    return x.astype(np.float32)


def loud_then_quiet(T, sr, seed=0):
    """0 dBFS noise, then -65 dBFS noise: the quiet blocks behind the loud passage must keep their energy"""
    g = np.random.RandomState(seed)
    x = g.uniform(-1.0, 1.0, T)
    x[T // 2:] *= 10.0 ** (-65.0 / 20.0)
    return x.astype(np.float32)


# ---- the cases both test files run: the host file asserts the margin on them, the GPU file the kernel's accuracy ---------------------------
SPAN = 8192                 # the samples per workgroup the library reports (psnd_loudness_span; asserted equal in both files)


def cases():
    """(name, sr, T or None, channels): every seam of the kernel at sr = 8000 (B = 3200, H = 800 does not divide the span)"""
    B, H = block(8000)
    out = [('noise', 8000, T, None) for T in (B - 1, B, B + H - 1, B + H, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1, 3 * SPAN + 17)]
    return out + [('noise', 22050, 4 * 8192 + 5, None), ('noise', 8000, 2 * SPAN + 1, 2), ('noise', 8000, SPAN + 1, 5),
                  ('two_level', 16000, None, None), ('loud_quiet', 8000, 3 * SPAN + 17, None)]


def case_input(name, sr, T, C, seed=11):
    if name == 'noise':
        return gated_noise(seed + (T % 97), T, sr, C)
    if name == 'two_level':
        return two_level_sine(sr)
    return loud_then_quiet(T, sr)
