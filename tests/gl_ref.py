"""The yardstick of the Griffin-Lim tests: the definition of include/psnd.h restated independently of pytorch_sound_amd.kernels (test
infrastructure, never imported by the product).

    start(mag, phase, frames, dtype)                       X0 = S (cos phi, sin phi) or (S, 0)
    step(mag, cre, cim, pre, pim, alpha, eps, frames, dtype)   one phase step; (xre, xim) float64 arrays (N, K, F)
    partial(mag, cre, cim, chunk, frames, dtype)           the per-chunk sums of (|C| - S)^2 and S^2, (N, chunks, 2), by a plain loop that
                                                           adds element after element
    loop(mag, stft, n_iter, momentum, phase, dtype)        the whole loop between stft.inverse_complex / transform_complex on CPU tensors of
                                                           `dtype`; (waveform (N, (F - 1) hop), conv (n_iter, N)) as float64 arrays

dtype=np.float64 is the yardstick.  dtype=np.float32 is the float32 VARIANT: every operation of the definition rounded to float32 (numpy's
correctly rounded hypot, cos, sin and division), the sums added in float32 in element order, and in `loop` the host transforms run on float32
tensors.  Its distance from the float64 run is what float32 arithmetic costs on a case; the GPU tests bound the kernel by a multiple of it.
The step is elementwise, so a numpy expression over the planes IS the loop over the elements: each element sees the same IEEE operations in
the same order.  Only the sums have an order, and `partial` spells it out.
"""
import numpy as np

EPS = 1e-16


def _live(shape, frames):
    N, _, F = shape
    Fn = np.full(N, F) if frames is None else np.clip(np.asarray(frames, dtype=np.int64).reshape(N), 0, F)
    return np.arange(F)[None, None, :] < Fn[:, None, None]


def _clean(a, live, dt):
    """the plane in dtype dt with what lies behind an item's frames replaced by zeros: the definition never reads it"""
    return np.where(live, np.asarray(a), 0).astype(dt)


def start(mag, phase=None, frames=None, dtype=np.float64):
    dt = dtype
    live = _live(np.shape(mag), frames)
    S = _clean(mag, live, dt)
    if phase is None:
        return S.astype(np.float64), np.zeros(S.shape)
    phi = _clean(phase, live, dt)
    with np.errstate(invalid='ignore', over='ignore'):
        xr, xi = S * np.cos(phi), S * np.sin(phi)
    return np.where(live, xr, 0.0).astype(np.float64), np.where(live, xi, 0.0).astype(np.float64)


def step(mag, cre, cim, pre=None, pim=None, alpha=0.0, eps=EPS, frames=None, dtype=np.float64):
    dt = dtype
    live = _live(np.shape(mag), frames)
    S, cr, ci = (_clean(a, live, dt) for a in (mag, cre, cim))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        tr, ti = cr, ci
        if pre is not None:
            tr = cr - dt(alpha) * _clean(pre, live, dt)
            ti = ci - dt(alpha) * _clean(pim, live, dt)
        den = np.hypot(tr, ti) + dt(eps)
        xr, xi = S * (tr / den), S * (ti / den)
    assert xr.dtype == dt
    return np.where(live, xr, 0).astype(np.float64), np.where(live, xi, 0).astype(np.float64)


def partial(mag, cre, cim, chunk, frames=None, dtype=np.float64):
    dt = dtype
    shape = np.shape(mag)
    N, M = shape[0], shape[1] * shape[2]
    live = _live(shape, frames)
    S, cr, ci = (_clean(a, live, dt).reshape(N, M) for a in (mag, cre, cim))
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.hypot(cr, ci) - S
        dd, ss = d * d, S * S
    chunks = -(-M // chunk)
    out = np.zeros((N, chunks, 2))
    lv = np.broadcast_to(live, shape).reshape(N, M)
    for n in range(N):
        for c in range(chunks):
            a, b = dt(0), dt(0)
            for e in range(c * chunk, min((c + 1) * chunk, M)):
                if lv[n, e]:
                    a, b = dt(a + dd[n, e]), dt(b + ss[n, e])
            out[n, c] = float(a), float(b)
    return out


def loop(mag, stft, n_iter, momentum, phase=None, dtype=np.float64):
    """mag, phase: (N, K, F) arrays.  The transforms are the host paths of `stft` on CPU tensors of `dtype`."""
    import torch
    dt = dtype
    tt = torch.float64 if dt is np.float64 else torch.float32
    alpha = momentum / (1.0 + momentum)
    S = np.asarray(mag).astype(dt)

    def inverse(X):
        return stft.inverse_complex(torch.from_numpy(np.ascontiguousarray(X[0].astype(dt))), torch.from_numpy(np.ascontiguousarray(X[1].astype(dt))))

    X = start(S, phase, None, dt)
    P, conv = None, []
    with torch.no_grad():
        for _ in range(n_iter):
            y = inverse(X)
            assert y.dtype == tt
            C = tuple(c.numpy() for c in stft.transform_complex(y))
            assert C[0].dtype == dt
            X = step(S, C[0], C[1], None if P is None else P[0], None if P is None else P[1], alpha, EPS, None, dt)
            P = C
            d = np.hypot(C[0], C[1]) - S
            num, den = (d * d).sum(axis=(1, 2), dtype=dt), (S * S).sum(axis=(1, 2), dtype=dt)
            conv.append(np.where(den > 0, np.sqrt(num / np.maximum(den, np.finfo(dt).tiny)), 0).astype(np.float64))
        y = inverse(X).double().numpy()
    return y, np.array(conv).reshape(n_iter, S.shape[0])


def planes(N, K, F, seed=0, count=5):
    """`count` float32 planes (N, K, F): the first non-negative (a magnitude), the others normal"""
    rs = np.random.RandomState(7000 + seed)
    out = [rs.uniform(0.0, 2.0, (N, K, F)).astype(np.float32)]
    out += [rs.randn(N, K, F).astype(np.float32) for _ in range(count - 1)]
    return out


def clip(T, seed=0):
    """two tones plus noise, float32 (T,)"""
    rs = np.random.RandomState(9000 + seed)
    t = np.arange(T)
    return (0.5 * np.sin(2 * np.pi * 0.05 * t + 0.3) + 0.3 * np.sin(2 * np.pi * 0.12 * t + 1.0) + 0.05 * rs.randn(T)).astype(np.float32)


def rel_err(y, ref):
    """max |y - ref| / max |ref| over all arrays of a case (y, ref: an array or a tuple of arrays); every element is compared.  Non-finite
    reference elements must be matched in kind and are left out."""
    ys = y if isinstance(y, (tuple, list)) else (y,)
    rs = ref if isinstance(ref, (tuple, list)) else (ref,)
    assert len(ys) == len(rs)
    top, worst = 0.0, 0.0
    for a, b in zip(ys, rs):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        assert a.shape == b.shape, (a.shape, b.shape)
        ok = np.isfinite(b)
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~ok & ~np.isnan(b)], b[~ok & ~np.isnan(b)]), 'non-finite elements differ'
        top = max(top, np.abs(b[ok]).max(initial=0.0))
        worst = max(worst, np.abs(a[ok] - b[ok]).max(initial=0.0))
    return float(worst if top == 0.0 else worst / top)
