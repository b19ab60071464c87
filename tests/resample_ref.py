"""Yardstick and bound of the sample-rate conversion tests (test infrastructure, never imported by the product).

Definition (include/psnd.h): for reduced factors up, down, a filter h of 2P + 1 values and a row x of T samples,

    y[m] = sum_i x[i] h[m down - i up + P]      over 0 <= i < T with 0 <= m down - i up + P <= 2P,      0 <= m < T_out,

T_out = ceil(T up / down) unless given.  The default h is firwin(2P + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up, P = 10 max(up, down):
then the sum is scipy.signal.resample_poly(x, up, down) with its zero padding (tests/test_resample_host.py holds the two together).  It is
written here as the direct sum in float64, not through scipy: output m meets the samples i = floor(c / up) - j, c = m down + P, j = 0, 1, ...,
through the values h[c mod up + j up].  The adjoint, gx[i] = sum_m gy[m] h[m down - i up + P], scatters the same products.

Bound per output:  |got[m] - y64[m]| <= (K_m + 3) 2^-24 sum_i |x[i]| |h32[k]| + 2^-149,   K_m = the number of products of output m.
  A float32 sum of K products rounds every product and every addition once (an fma one of the two): at most K 2^-24 of sum |x| |h| to first
  order, in any order of summation.  The three more are the rounding of the taps to float32 (the yardstick uses the float64 taps), the
  rounding of the result and the second-order terms; 2^-149 is the smallest subnormal, for sums that underflow.
"""
import math

import numpy as np
from scipy import signal

RATIOS = ((2, 1), (1, 2), (3, 2), (2, 3), (160, 147), (147, 320), (320, 441), (441, 320))


def taps(up, down):
    g = math.gcd(up, down)
    up, down = up // g, down // g
    big = max(up, down)
    return signal.firwin(2 * 10 * big + 1, 1.0 / big, window=('kaiser', 5.0)) * up


def out_len(T, up, down):
    return -(-T * up // down)


def max_products(n_taps, up):
    """K: the largest number of products of one output, ceil(n_taps / up)"""
    return -(-n_taps // up)


def _products(T, n_taps, up, down, T_out):
    """(i, k, ok): sample index, tap index and validity of product j of output m, each (T_out, K)"""
    P = n_taps // 2
    c = np.arange(T_out, dtype=np.int64) * down + P
    ihi = c // up
    phi = c - ihi * up
    j = np.arange(-(-n_taps // up), dtype=np.int64)
    i = ihi[:, None] - j[None, :]
    k = phi[:, None] + j[None, :] * up
    ok = (i >= 0) & (i < T) & (k < n_taps)
    return np.where(ok, i, 0), np.where(ok, k, 0), ok


def resample(x, up, down, h=None, T_out=None):
    """the definition along the last axis, in float64"""
    x = np.asarray(x).astype(np.float64)
    h = taps(up, down) if h is None else np.asarray(h, dtype=np.float64)
    T = x.shape[-1]
    T_out = out_len(T, up, down) if T_out is None else T_out
    if T == 0 or T_out == 0:
        return np.zeros(x.shape[:-1] + (T_out,))
    i, k, ok = _products(T, h.size, up, down, T_out)
    return np.where(ok, x[..., i] * h[k], 0.0).sum(axis=-1)


def adjoint(gy, up, down, T, h=None):
    """gx[i] = sum_m gy[m] h[m down - i up + P]: the gradient of <resample(x, up, down, h), gy> in x of length T, the same products scattered"""
    gy = np.asarray(gy).astype(np.float64)
    h = taps(up, down) if h is None else np.asarray(h, dtype=np.float64)
    gx = np.zeros(gy.shape[:-1] + (T,))
    if T == 0 or gy.shape[-1] == 0:
        return gx
    i, k, ok = _products(T, h.size, up, down, gy.shape[-1])
    flat, out = gy.reshape(-1, gy.shape[-1]), gx.reshape(-1, T)
    for r in range(flat.shape[0]):
        np.add.at(out[r], i[ok], (flat[r][:, None] * h[k])[ok])
    return gx


def bound(x, h32, up, down, T_out):
    """the derived bound per output of the float32 sum against the float64 one (module docstring)"""
    x = np.abs(np.asarray(x).astype(np.float64))
    h = np.abs(np.asarray(h32, dtype=np.float32).astype(np.float64))
    T = x.shape[-1]
    if T == 0 or T_out == 0:
        return np.full(x.shape[:-1] + (T_out,), 2.0 ** -149)
    i, k, ok = _products(T, h.size, up, down, T_out)
    mass = np.where(ok, x[..., i] * h[k], 0.0).sum(axis=-1)
    return (ok.sum(axis=-1) + 3) * 2.0 ** -24 * mass + 2.0 ** -149


def excess(got, want, bd):
    """largest |got - want| / bound over the elements (<= 1 passes)"""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    assert got.shape == want.shape == bd.shape, (got.shape, want.shape, bd.shape)
    err = np.abs(got - want)
    if not np.isfinite(err).all():
        return float('inf')
    return float(np.max(np.where(err == 0, 0.0, err / bd)))


def signal_rows(seed, N, T):
    """float32 rows of T samples, row r of kind r mod 4: noise, an impulse at sample 0, an impulse at the last sample, a constant"""
    g = np.random.RandomState(seed)
    x = (0.3 * g.randn(N, T)).astype(np.float32)
    for r in range(N):
        kind = r % 4
        if kind in (1, 2):
            x[r] = 0.0
            if T:
                x[r, 0 if kind == 1 else T - 1] = 1.0
        elif kind == 3:
            x[r] = 0.25
    return x
