"""The yardstick of the mel-inverse tests: the definition of include/psnd.h restated independently of pytorch_sound_amd.kernels (test
infrastructure, never imported by the product).

    plan(W, n_iter_max)                                    {A fp32, d, cinv, c, L, step, beta fp32} - the sums term after term, ascending
    solve_frame(P, y, n_iter, log_kind, log_offset, dtype) ONE frame: y (M,) -> (x (K,), resid), every sum a plain loop over its terms
    solve(P, Y, n_iter, log_kind, log_offset, frames, dtype)   Y (N, M, F) -> (x (N, K, F), resid (N, F)) as float64 arrays

dtype=np.float64 is the yardstick.  dtype=np.float32 is the float32 VARIANT: d, cinv, step and every operation of the definition rounded
to float32 (numpy's correctly rounded exp, power, sqrt and division; products rounded before they are added), the sums added in float32 in
ascending index.  Its distance from the float64 run is what float32 arithmetic costs on a case; the GPU tests bound the kernel by a multiple
of it.  `solve` IS the loop over the frames: frames never interact, and each sum is built term after term by numpy expressions over the
frame axis, so every frame sees the IEEE operations of `solve_frame` in the same order (tests/test_mel_inverse_host.py holds the two to the
same bits).  A term whose weight is zero adds an exact zero: walking all indices gives the bits of walking the band.
"""
import math

import numpy as np

LOG_NONE, LOG_E, LOG_10 = 0, 1, 2


def plan(W, n_iter_max=64):
    W = np.asarray(W, dtype=np.float32).astype(np.float64)
    assert W.ndim == 2 and np.isfinite(W).all() and (W >= 0).all()
    M, K = W.shape
    s = np.zeros(M)
    for k in range(K):
        s = s + W[:, k]
    d = np.array([1.0 / v if v > 0 else 0.0 for v in s])
    A = (d[:, None] * W).astype(np.float32)
    A64 = A.astype(np.float64)
    c = np.zeros(K)
    for m in range(M):
        c = c + A64[m]
    cinv = np.array([1.0 / v if v > 0 else 0.0 for v in c])
    rows = np.zeros(M)
    for k in range(K):
        rows = rows + A64[:, k] * c[k]
    L = float(rows.max())
    beta, t = [], 1.0
    for _ in range(n_iter_max):
        tn = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        beta.append((t - 1.0) / tn)
        t = tn
    return dict(A=A, d=d, cinv=cinv, c=c, L=L, step=1.0 / L if L > 0 else 0.0, beta=np.array(beta, dtype=np.float32))


def _undo_log(y, log_kind, off, dt):
    if log_kind == LOG_E:
        return np.exp(y) - dt(off)
    if log_kind == LOG_10:
        return np.power(dt(10.0), y) - dt(off)
    assert log_kind == LOG_NONE
    return y


def solve_frame(P, y, n_iter, log_kind=LOG_NONE, log_offset=0.0, dtype=np.float64):
    dt = dtype
    A = P['A'].astype(dt)
    M, K = A.shape
    d, cinv, step = P['d'].astype(dt), P['cinv'].astype(dt), dt(P['step'])
    zero = dt(0)
    with np.errstate(invalid='ignore', over='ignore'):
        lin = _undo_log(np.asarray(y).astype(dt), log_kind, log_offset, dt)
        b = [dt(d[m] * max(lin[m], zero)) if not np.isnan(lin[m]) else dt(d[m] * zero) for m in range(M)]

        def A_times(v):
            out = []
            for m in range(M):
                acc = zero
                for k in range(K):
                    acc = dt(acc + dt(A[m, k] * v[k]))
                out.append(acc)
            return out

        def At_times(v):
            out = []
            for k in range(K):
                acc = zero
                for m in range(M):
                    acc = dt(acc + dt(A[m, k] * v[m]))
                out.append(acc)
            return out

        x = [dt(cinv[k] * a) for k, a in enumerate(At_times(b))]
        z = list(x)
        for i in range(n_iter):
            be = dt(P['beta'][i])
            r = [dt(a - b[m]) for m, a in enumerate(A_times(z))]
            g = At_times(r)
            xn = [max(dt(z[k] - dt(step * g[k])), zero) for k in range(K)]
            z = [dt(xn[k] + dt(be * dt(xn[k] - x[k]))) for k in range(K)]
            x = xn
        r = [dt(a - b[m]) for m, a in enumerate(A_times(x))]
        rr = bb = zero
        for m in range(M):
            rr, bb = dt(rr + dt(r[m] * r[m])), dt(bb + dt(b[m] * b[m]))
        resid = float(np.sqrt(dt(rr / bb))) if bb > 0 else 0.0
    return np.array(x, dtype=np.float64), resid


def solve(P, Y, n_iter, log_kind=LOG_NONE, log_offset=0.0, frames=None, dtype=np.float64):
    dt = dtype
    A = P['A'].astype(dt)
    M, K = A.shape
    Y = np.asarray(Y)
    N, _, F = Y.shape
    assert Y.shape[1] == M
    Fn = np.full(N, F) if frames is None else np.clip(np.asarray(frames, dtype=np.int64).reshape(N), 0, F)
    live = (np.arange(F)[None, :] < Fn[:, None]).reshape(1, N * F)
    d, cinv, step = P['d'].astype(dt)[:, None], P['cinv'].astype(dt)[:, None], dt(P['step'])
    # frames side by side: (M, N F) and (K, N F); what lies behind an item's frames is replaced by zeros, the definition never reads it
    Yc = np.where(live, np.moveaxis(Y, 1, 0).reshape(M, N * F), 0).astype(dt)
    rows_used = [k for k in range(K) if A[:, k].any()]
    cols_used = [m for m in range(M) if A[m].any()]

    def A_times(v):
        acc = np.zeros((M, v.shape[1]), dtype=dt)
        for k in rows_used:                                     # a bin no filter reaches adds exact zeros
            acc = acc + A[:, k, None] * v[k][None, :]
        return acc

    def At_times(v):
        acc = np.zeros((K, v.shape[1]), dtype=dt)
        for m in cols_used:
            acc = acc + A[m, :, None] * v[m][None, :]
        return acc

    with np.errstate(invalid='ignore', over='ignore'):
        lin = _undo_log(Yc, log_kind, log_offset, dt)
        b = d * np.fmax(lin, dt(0))
        b = np.where(np.isnan(lin), d * dt(0), b)
        x = cinv * At_times(b)
        z = x
        for i in range(n_iter):
            be = dt(P['beta'][i])
            r = A_times(z) - b
            g = At_times(r)
            xn = np.fmax(z - step * g, dt(0))
            z = xn + be * (xn - x)
            x = xn
        assert x.dtype == dt and z.dtype == dt and b.dtype == dt
        r = A_times(x) - b
        rr, bb = np.zeros(N * F, dtype=dt), np.zeros(N * F, dtype=dt)
        for m in range(M):
            rr, bb = rr + r[m] * r[m], bb + b[m] * b[m]
        resid = np.where(bb > 0, np.sqrt(rr / np.where(bb > 0, bb, dt(1))), dt(0))
    x = np.where(live, x, 0).astype(np.float64)
    resid = np.where(live[0], resid, 0).astype(np.float64)
    return np.moveaxis(x.reshape(K, N, F), 0, 1).copy(), resid.reshape(N, F)


def spectra(N, K, F, seed=0, peaks=True):
    """non-negative float64 spectra (N, K, F): a smooth envelope, plus narrow peaks that move from frame to frame"""
    rs = np.random.RandomState(3000 + seed)
    k = np.arange(K)[None, :, None] / max(K - 1, 1)
    X = (0.2 + rs.rand(N, 1, F)) * np.exp(-3.0 * k * rs.rand(N, 1, F)) * (1.0 + 0.5 * np.cos(2 * np.pi * k * (1 + 4 * rs.rand(N, 1, F))))
    if peaks:
        for _ in range(4):
            pos = rs.randint(0, K, (N, 1, F))
            X = X + 3.0 * rs.rand(N, 1, F) * (np.arange(K)[None, :, None] == pos)
    return np.maximum(X, 0.0)


def mels(W, X):
    """Y = W X in float64, rounded to float32: what a test feeds"""
    return np.einsum('mk,nkf->nmf', np.asarray(W, dtype=np.float64), X).astype(np.float32)


def rel_err(y, ref):
    """max |y - ref| / max |ref|; every element is compared.  Non-finite reference elements must be matched in kind and are left out."""
    a, b = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    ok = np.isfinite(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~ok & ~np.isnan(b)], b[~ok & ~np.isnan(b)]), 'non-finite elements differ'
    top = np.abs(b[ok]).max(initial=0.0)
    worst = np.abs(a[ok] - b[ok]).max(initial=0.0)
    return float(worst if top == 0.0 else worst / top)
