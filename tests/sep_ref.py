"""The yardstick of the separation metrics (test infrastructure, never imported by the product): SNR / SI-SDR / SD-SDR by the definition of
include/psnd.h in numpy float64, TWO-PASS - the means first, then the explicit scaled-target and residual vectors and their energies, so
no energy is ever a difference of sums - the permutation by brute force, the gradients by torch float64 autograd on the CPU over the
same explicit formulas, and mixing at an SNR.  Everything evaluates the float32 samples the kernel gets.

It also builds the inputs of the GPU cases (`CASES`), so that tests/test_sep_host.py can assert on the CPU what the GPU tests rely on:
every yardstick value lies below CAP_DB, and wherever a permutation is searched the best and the second-best sums are GAP_DB apart
(the planted tie excepted, which is decided by rule)."""
import itertools
import math
from collections import namedtuple

import numpy as np

SPAN = 8192                      # psnd_sep_span(): asserted equal by the tests
KINDS = ('snr', 'si_sdr', 'sd_sdr')
EPS = float(np.finfo(np.float32).eps)
CAP_DB = 60.0                    # the ratio cap of the 1e-4 dB bound
GAP_DB = 1e-3                    # best against second-best permutation sum

Reading = namedtuple('Reading', 'value perm pair gap')      # float64 (B, S), int (B, S), float64 (B, S, S), smallest best - second best


def lengths_of(lengths, B, T):
    if lengths is None:
        return [T] * B
    return [min(max(int(v), 0), T) for v in lengths]


def pair_value(kind, e, s, zero_mean, eps=EPS):
    """one pair: 1-D float64 rows already cut to the length"""
    if zero_mean and e.size:
        e, s = e - e.mean(), s - s.mean()
    if kind == 'snr':
        tgt, res = s, s - e
    else:
        a = (float(e @ s) + eps) / (float(s @ s) + eps)
        tgt = a * s
        res = tgt - e if kind == 'si_sdr' else s - e
    num, den = float(tgt @ tgt) + eps, float(res @ res) + eps
    if den == 0.0:
        return math.nan if num == 0.0 else math.inf
    return 10.0 * math.log10(num / den) if num > 0.0 else -math.inf


def best_perm(pv):
    """(perm, gap) of a float64 pair matrix: the lexicographically first permutation of the largest sum (added in ascending i), and the
    distance of that sum to the largest sum of another permutation (inf for S = 1)"""
    S = pv.shape[0]
    sums = []
    for p in itertools.permutations(range(S)):
        t = 0.0
        for i in range(S):
            t += float(pv[i, p[i]])
        sums.append((t, p))
    top = max(t for t, _ in sums)
    first = next(p for t, p in sums if t == top)
    rest = [t for t, p in sums if p != first]
    return list(first), (top - max(rest) if rest else math.inf)


def measure(est, target, kind, zero_mean=False, eps=EPS, lengths=None, pit=False):
    est, target = np.asarray(est), np.asarray(target)
    B, S, T = est.shape
    lens = lengths_of(lengths, B, T)
    value, perm, pair, gap = np.zeros((B, S)), np.tile(np.arange(S), (B, 1)), np.zeros((B, S, S)), math.inf
    for b in range(B):
        e, s = est[b, :, :lens[b]].astype(np.float64), target[b, :, :lens[b]].astype(np.float64)
        if not (np.isfinite(e).all() and np.isfinite(s).all()):
            value[b], pair[b] = np.nan, np.nan
            continue
        for i in range(S):
            for j in range(S):
                pair[b, i, j] = pair_value(kind, e[i], s[j], zero_mean, eps)
        if pit:
            perm[b], g = best_perm(pair[b])
            gap = min(gap, g)
        value[b] = pair[b][np.arange(S), perm[b]]
    return Reading(value, perm, pair, gap)


def gradients(est, target, kind, zero_mean, perm, eps=EPS, lengths=None, g_value=None, g_loss=None):
    """float64 (d / d est, d / d target) of sum(g_value value) + g_loss (-mean value) with the matching `perm` held fixed: torch autograd on
    the CPU over the two-pass formulas"""
    import torch
    B, S, T = est.shape
    lens = lengths_of(lengths, B, T)
    E = torch.from_numpy(np.asarray(est, dtype=np.float64)).requires_grad_(True)
    G = torch.from_numpy(np.asarray(target, dtype=np.float64)).requires_grad_(True)
    rows = []
    for b in range(B):
        for i in range(S):
            e, s = E[b, i, :lens[b]], G[b, int(perm[b][i]), :lens[b]]
            if zero_mean and lens[b]:
                e, s = e - e.mean(), s - s.mean()
            if kind == 'snr':
                tgt, res = s, s - e
            else:
                a = (e.dot(s) + eps) / (s.dot(s) + eps)
                tgt = a * s
                res = tgt - e if kind == 'si_sdr' else s - e
            rows.append(10.0 * torch.log10((tgt.dot(tgt) + eps) / (res.dot(res) + eps)))
    value = torch.stack(rows).reshape(B, S)
    total = torch.zeros((), dtype=torch.float64)
    if g_value is not None:
        total = total + (torch.from_numpy(np.asarray(g_value, dtype=np.float64)) * value).sum()
    if g_loss is not None:
        total = total + float(g_loss) * (-value.mean())
    total.backward()
    return E.grad.numpy(), G.grad.numpy()


def mix(x, z, snr, lengths=None):
    """(float64 x + g z before the length and x behind it, float64 g) per row of (R, T); g = 0 for a silent or non-finite row"""
    x, z = np.asarray(x), np.asarray(z)
    R, T = x.shape
    lens = lengths_of(lengths, R, T)
    snr = np.broadcast_to(np.asarray(snr, dtype=np.float64).reshape(-1), (R,))
    y, g = x.astype(np.float64).copy(), np.zeros(R)
    for r in range(R):
        a, b = x[r, :lens[r]].astype(np.float64), z[r, :lens[r]].astype(np.float64)
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        xx, zz = float(a @ a), float(b @ b)
        if xx > 0.0 and zz > 0.0:
            g[r] = math.sqrt(xx / zz) * 10.0 ** (-snr[r] / 20.0)
            y[r, :lens[r]] = a + g[r] * b
    return y, g


# ---- the inputs of the GPU cases ------------------------------------------------------------------------------------------------------------
def sources(seed, B, S, T, perms=None, noise_db=None, dc=0.0):
    """(est, target) float32 (B, S, T): targets are white noise at distinct levels, estimate i of item b is target perms[b][i] plus noise
    noise_db[i] dB below it (distinct levels), both with a DC offset of `dc` times the rms"""
    rs = np.random.RandomState(seed)
    level = 0.08 * 0.8 ** np.arange(S)                   # one sample at 3 sigma still reads below CAP_DB in si_sdr: 10 log10(e^2 / eps)
    tgt = rs.randn(B, S, T) * level[None, :, None]
    noise_db = [18.0 + 7.0 * i for i in range(S)] if noise_db is None else noise_db
    est = np.empty_like(tgt)
    for b in range(B):
        p = list(range(S)) if perms is None else perms[b]
        for i in range(S):
            est[b, i] = tgt[b, p[i]] + rs.randn(T) * level[p[i]] * 10.0 ** (-noise_db[i] / 20.0)
    if dc:
        tgt = tgt + dc * level[None, :, None]
        est = est + dc * level[None, :, None] * 1.1
    return est.astype(np.float32), tgt.astype(np.float32)


def mixed_lengths(B, T):
    """{0, 1, T - 1, T} and one in the middle, as far as B rows go"""
    return [T, T - 1, 1, 0, T // 2 + 1][:B]


SEAM_T = (1, 3, SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 3)
SHAPES = [(B, S) for S in (1, 2, 3, 4) for B in (1, 5)]
S3_PERMS = [list(p) for p in itertools.permutations(range(3))]
S4_PERM = [[2, 3, 1, 0], [1, 0, 3, 2]]


def case(name):
    """(est, target, lengths, pit) of a named GPU case"""
    kind, *arg = name.split(':')
    if kind == 'seam':                                   # 'seam:T'
        T = int(arg[0])
        S = 1 + SEAM_T.index(T) % 4
        est, tgt = sources(100 + T % 97, 2, S, T)
        return est, tgt, None, S > 1
    if kind == 'shape':                                  # 'shape:B:S'
        B, S = int(arg[0]), int(arg[1])
        T = SPAN + 5
        if B > 1:                                        # {0, 1, T - 1, T} in one batch, matched as given: an item of no or one sample
            est, tgt = sources(200 + 10 * B + S, B, S, T)    # has no best permutation (the planted tie below covers that rule)
            return est, tgt, mixed_lengths(B, T), False
        est, tgt = sources(200 + 10 * B + S, B, S, T, perms=[list(np.roll(np.arange(S), 1))])
        return est, tgt, None, S > 1
    if kind == 'dc':                                     # a DC offset of twice the rms
        est, tgt = sources(300, 2, 2, 3001, dc=2.0)
        return est, tgt, None, False
    if kind == 'pit3':                                   # each of the six permutations planted once
        est, tgt = sources(400, 6, 3, 2 * SPAN + 1, perms=S3_PERMS)
        return est, tgt, None, True
    if kind == 'pit4':
        est, tgt = sources(500, 2, 4, SPAN + 7, perms=S4_PERM)
        return est, tgt, [SPAN + 7, SPAN - 3], True
    if kind == 'tie':                                    # two bit-identical estimates, and an item of no samples: decided by rule
        est, tgt = sources(600, 2, 3, 4099, perms=[[1, 2, 0], [2, 0, 1]])
        est[0, 1] = est[0, 0]
        return est, tgt, [4099, 0], True
    if kind == 'full':                                   # (4, 2, 30 s at 44.1 kHz)
        est, tgt = sources(700, 4, 2, 30 * 44100, perms=[[0, 1], [1, 0], [1, 0], [0, 1]], noise_db=[25.0, 40.0])
        return est, tgt, [30 * 44100, 30 * 44100 - 1, 1000001, 30 * 44100], True
    raise KeyError(name)


CASES = ['seam:%d' % T for T in SEAM_T] + ['shape:%d:%d' % bs for bs in SHAPES] + ['dc', 'pit3', 'pit4', 'tie', 'full']
CONFIGS = [(k, zm) for k in KINDS for zm in (False, True)]
FULL_CONFIGS = [('si_sdr', True), ('snr', False)]       # what the full-size case is run with


def high_ratio_case():
    """one item near 100 dB: checked against its own bound only"""
    est, tgt = sources(800, 1, 1, 3 * SPAN + 2, noise_db=[100.0])
    return est * 8.0, tgt * 8.0                          # a power of two, exact: an rms of 0.64 keeps eps out of the ratio


def moment_bound_db(v_db, m_plus_d):
    """the bound of the derivation in tests/test_gpu_sep_metrics.py on the error in dB of a value near v_db: the moments carry a relative
    error of (m + d) 2^-53, the residual energy is a difference of them, amplified by 4 10^(v / 10); 10 / ln 10 dB per unit of relative
    error; plus half an fp32 ulp of the value"""
    ulp = 2.0 ** (math.floor(math.log2(max(abs(v_db), 1e-30))) - 24)
    return (10.0 / math.log(10.0)) * 4.0 * 10.0 ** (v_db / 10.0) * m_plus_d * 2.0 ** -53 + ulp
