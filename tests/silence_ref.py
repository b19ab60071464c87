"""Yardstick of the silence detector (include/psnd.h, utils/silence.py): plain Python on numpy rows, nothing shared with the code under test.

Energies are math.fsum over the float64 squares of a window (exactly rounded), the merge is the sequential rule of the definition.  Every
input the tests build carries a MARGIN: no window's energy lies within `margin * theta` of the threshold theta (for theta = 0: a window is
all zeros, or its energy is at least TINY), so the float32 dot product of the reference, the block-local float64 sums of the kernels and
the exact sum here cannot disagree on a decision, and all comparisons are exact equality of integers."""
import math

import numpy as np

MARGIN = 1e-3
TINY = 1e-12            # theta = 0: the smallest energy a window with a non-zero sample may have (one sample of 2^-16 has 2.3e-10)


def theta_of(L, db):
    return 0.0 if db == -math.inf else L * 10.0 ** (db / 10.0)


def starts(T, L, s):
    if T < L:
        return []
    out = list(range(0, T - L + 1, s))
    if (T - L) % s:
        out.append(T - L)
    return out


def cap(T, L):
    return 0 if T < L else (T - L) // (L + 1) + 1


def energies(x, L, s):
    """[(start, E, holds a non-finite sample)]"""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    sq = (np.where(fin, x, 0.0) ** 2).tolist()
    bad = np.concatenate(([0], np.cumsum(~fin))).tolist()
    return [(i, math.fsum(sq[i:i + L]), bad[i + L] - bad[i] > 0) for i in starts(len(sq), L, s)]


def margin(x, L, s, db):
    """the smallest |E - theta| / theta over the windows without a non-finite sample (inf if there are none); for theta = 0 the smallest
    non-zero energy divided by TINY"""
    th = theta_of(L, db)
    m = math.inf
    for _, E, bad in energies(x, L, s):
        if bad:
            continue
        if th == 0.0:
            if E != 0.0:
                m = min(m, E / TINY)
        else:
            m = min(m, abs(E - th) / th)
    return m


def assert_margin(x, L, s, db, least=MARGIN):
    m = margin(x, L, s, db)
    assert m >= (1.0 if theta_of(L, db) == 0.0 else least), 'a window within %.3g of the threshold (L=%d s=%d dB=%r)' % (m, L, s, db)
    return m


def detect_silence(x, L, db, s=1):
    th = theta_of(L, db)
    silent = [i for i, E, bad in energies(x, L, s) if not bad and E <= th]
    out = []
    p = None
    for k in silent:
        if p is None or (k != p + s and k > p + L):
            out.append([k, k + L])
        else:
            out[-1][1] = k + L
        p = k
    return out


def detect_nonsilent(x, L, db, s=1):
    T = len(x)
    silent = detect_silence(x, L, db, s)
    if not silent:
        return [[0, T]]
    if silent[0] == [0, T]:
        return []
    edges = [0] + [v for r in silent for v in r] + [T]          # gaps lie between an end and the next start
    out = [[edges[k], edges[k + 1]] for k in range(0, len(edges), 2)]
    if out[-1][0] == T:
        out.pop()
    if out[0] == [0, 0]:
        out.pop(0)
    return out


def packed(rows, L, db, s, lengths=None):
    """(count, ranges) as kernels.silence_ranges returns them for the rows of a batch: int32 (N,), int64 (N, cap, 2) filled with -1"""
    T = len(rows[0])
    count = np.zeros(len(rows), dtype=np.int32)
    ranges = np.full((len(rows), cap(T, L), 2), -1, dtype=np.int64)
    for n, row in enumerate(rows):
        r = detect_silence(row[:T if lengths is None else lengths[n]], L, db, s)
        count[n] = len(r)
        if r:
            ranges[n, :len(r)] = r
    return count, ranges


# ---- input builders ------------------------------------------------------------------------------------------------------------------------
def gated(seed, T, spans, quiet='noise'):
    """float32 row of T samples: loud noise (multiples of 1/256 with 0.25 <= |v| < 1) outside `spans`, and inside the [a, b) of `spans` quiet
    noise (multiples of 2^-16, |v| <= 2^-13: far below -60 dB) or exact zeros (quiet='zero').  Few distinct values: the fixture compresses."""
    r = np.random.RandomState(seed)
    x = (r.randint(64, 256, T) * r.choice((-1, 1), T) / 256.0).astype(np.float32)
    for a, b in spans:
        n = max(0, min(b, T) - max(a, 0))
        x[max(a, 0):min(b, T)] = 0.0 if quiet == 'zero' else (r.randint(-8, 9, n) / 65536.0).astype(np.float32)
    return x


def random_spans(seed, T, L, n=4):
    """n quiet spans of lengths around L (some too short to hold a window) at random places"""
    r = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        w = int(r.randint(max(1, L // 2), 3 * L + 2))
        a = int(r.randint(0, max(1, T - w + 1)))
        out.append((a, a + w))
    return out


def with_margin(build, L, s, db, tries=400, also=()):
    """build(seed) for the first seed whose row keeps the margin, also when it is cut to each of the lengths `also`"""
    for seed in range(tries):
        x = build(seed)
        m = min(margin(x[:n], L, s, db) for n in (len(x),) + tuple(also))
        if m >= (1.0 if theta_of(L, db) == 0.0 else MARGIN):
            return x
    raise AssertionError('no seed keeps the margin (L=%d s=%d dB=%r)' % (L, s, db))


def bursts(T=5000, period=9):
    """zeros with one sample of 0.5 every `period`: with L = 3, s = 1 every gap holds one short silent range"""
    x = np.zeros(T, dtype=np.float32)
    x[4::period] = 0.5
    return x


ACC_BLOCKS, ACC_L = 8, 10


def loud_then_quiet(seed=0):
    """(x, dB): 4 x 1024 samples of amplitude 1, then 4 x 1024 of noise below 1e-5, and a threshold for L = 10, s = 1 that lies between the
    exact energy of a quiet window and what a row-long float64 prefix sum gives for it, while every window's exact energy (math.fsum) keeps
    a margin of 1e-6: the block-local sums must decide as the exact ones, a global prefix cannot."""
    T, L = ACC_BLOCKS * 1024, ACC_L
    r = np.random.RandomState(seed)
    x = np.ones(T, dtype=np.float32)
    x[T // 2:] = (r.uniform(-1e-5, 1e-5, T // 2)).astype(np.float32)
    exact = np.array([E for _, E, _ in energies(x, L, 1)])
    glob = global_prefix_energies(x, L)
    lo, hi = np.percentile(exact[T // 2:], (30, 70))       # a threshold in the middle of the quiet windows: both decisions occur among them
    order = np.argsort(-np.abs(glob - exact) / np.maximum(exact, 1e-300))
    for w in order:
        if w < T // 2 or not lo <= exact[w] <= hi or glob[w] <= 0:
            continue
        db = 10.0 * math.log10(math.sqrt(exact[w] * glob[w]) / L)
        th = theta_of(L, db)
        if (exact[w] <= th) != (glob[w] <= th) and np.min(np.abs(exact - th)) >= 1e-6 * th:
            return x, db
    raise AssertionError('no threshold separates the exact energies from the global prefix')


def global_prefix_energies(x, L):
    """what the definition must NOT be computed by: differences of one row-long float64 prefix sum"""
    P = np.concatenate(([0.0], np.cumsum(np.asarray(x, dtype=np.float64) ** 2)))
    return P[L:] - P[:-L]
