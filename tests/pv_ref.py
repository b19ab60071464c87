"""The yardstick of the phase vocoder tests: the definition of include/psnd.h as a plain loop over rows and output frames, independent of
pytorch_sound_amd.kernels (test infrastructure, never imported by the product).

    pv(re, im, rate, frames=None, dtype=np.float64)   the definition; (yre, yim) float64 arrays (rows, J)
        dtype=np.float32: the float32 VARIANT - float32 arctan2, hypot, interpolation and polar step, the angle differences summed in
        float64 and reduced modulo a turn before the polar step.  Its distance from the float64 run is what float32 arithmetic costs on a
        case; the GPU tests bound the kernel by a multiple of it.
        phase32=True (with float32): the phase summed as a plain float32 number - what a kernel must NOT do; kept to show the drift.
    pv_textbook(re, im, rate, n_fft, hop)             torchaudio's wording in float64: expected advance, wrap, plain cumsum
    frames(F, rate)                                   the count of j >= 0 with float(j) * rate < F, by counting
"""
import numpy as np

TWO_PI = 2.0 * np.pi


def frames(F, rate):
    """by the wording: count upward while float(j) * rate < F"""
    j = 0
    while float(j) * float(rate) < F:
        j += 1
    return j


def _arg(re, im, dt):
    """arg with arg 0 = 0, in dtype dt"""
    if re == 0 and im == 0:
        return dt(0)
    return np.arctan2(dt(im), dt(re))


def pv_row(xr, xi, rate, J, dtype=np.float64, phase32=False):
    """one row: xr, xi the valid part of the row (frames behind it count as zeros); J output slots, zeros behind the row's own count"""
    dt = dtype
    F = len(xr)
    yr, yi = np.zeros(J), np.zeros(J)
    lost = False
    phi = 0.0                                           # float64 sum of angle differences (exact differences of the dt angles)
    phi32 = np.float32(0)
    prev = None
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(J):
            t = float(j) * float(rate)
            if not t < F:
                break
            i = int(np.floor(t))
            alpha = dt(t - i)
            a = (dt(xr[i]), dt(xi[i]))
            b = (dt(xr[i + 1]), dt(xi[i + 1])) if i + 1 < F else (dt(0), dt(0))
            if j == 0:
                phi = float(_arg(a[0], a[1], dt))
                phi32 = np.float32(phi)
            else:
                phi += prev
                phi32 = np.float32(phi32 + np.float32(prev))
            prev = float(_arg(b[0], b[1], dt)) - float(_arg(a[0], a[1], dt))
            lost = lost or not (np.isfinite(a[0]) and np.isfinite(a[1]) and np.isfinite(b[0]) and np.isfinite(b[1]))
            if lost:
                yr[j] = yi[j] = np.nan
                continue
            mag = (dt(1) - alpha) * np.hypot(a[0], a[1]) + alpha * np.hypot(b[0], b[1])
            if dt is np.float64:
                ang = phi
            elif phase32:
                ang = phi32
            else:
                ang = dt(np.remainder(phi + np.pi, TWO_PI) - np.pi)
            yr[j], yi[j] = float(dt(mag) * np.cos(dt(ang))), float(dt(mag) * np.sin(dt(ang)))
    return yr, yi


def pv(re, im, rate, frames_per_row=None, dtype=np.float64, phase32=False, J=None):
    """re, im: (rows, F); frames_per_row: valid frames per row (clamped to [0, F]) or None.  (yre, yim), float64 (rows, J)"""
    re, im = np.asarray(re), np.asarray(im)
    R, F = re.shape
    J = frames(F, rate) if J is None else J
    yr, yi = np.zeros((R, J)), np.zeros((R, J))
    for r in range(R):
        Fn = F if frames_per_row is None else min(max(int(frames_per_row[r]), 0), F)
        yr[r], yi[r] = pv_row(re[r, :Fn], im[r, :Fn], rate, J, dtype, phase32)
    return yr, yi


def pv_textbook(re, im, rate, n_fft, hop):
    """torchaudio.functional.phase_vocoder / librosa.phase_vocoder restated in float64 for (K, F) arrays with K = n_fft // 2 + 1: the
    expected advance pi hop k / (K - 1) per bin is taken off the angle differences, the rest wrapped to [-pi, pi], the advance added back,
    then a plain cumsum.  One zero frame is appended, as both libraries do."""
    X = np.asarray(re, np.float64) + 1j * np.asarray(im, np.float64)
    K, F = X.shape
    adv = np.linspace(0.0, np.pi * hop, K)[:, None]
    steps = np.arange(0, F, rate, dtype=np.float64)
    Xp = np.concatenate((X, np.zeros((K, 2))), axis=1)
    i = np.floor(steps).astype(np.int64)
    alpha = steps - i
    a0, a1 = np.angle(Xp[:, i]), np.angle(Xp[:, i + 1])
    n0, n1 = np.abs(Xp[:, i]), np.abs(Xp[:, i + 1])
    d = a1 - a0 - adv
    d = d - TWO_PI * np.round(d / TWO_PI)
    d = d + adv
    acc = np.concatenate((np.angle(X[:, :1]), d[:, :-1]), axis=1).cumsum(axis=1)
    mag = alpha * n1 + (1.0 - alpha) * n0
    return mag * np.cos(acc), mag * np.sin(acc)


def seeded_spectrum(n, K, F, seed=0, scale=1.0):
    """(re, im) float32 (n K, F): smooth-ish random spectra - a few rotating partials per row plus noise, so that magnitudes vary and phases
    advance by all sorts of amounts"""
    rs = np.random.RandomState(4000 + seed)
    f = np.arange(F)
    rows = n * K
    X = np.zeros((rows, F), np.complex128)
    for _ in range(3):
        w = rs.uniform(-np.pi, np.pi, (rows, 1))
        amp = rs.uniform(0.1, 1.0, (rows, 1)) * (1.0 + 0.5 * np.sin(rs.uniform(0.01, 0.2, (rows, 1)) * f + rs.uniform(0, 6, (rows, 1))))
        X += amp * np.exp(1j * (w * f + rs.uniform(-np.pi, np.pi, (rows, 1))))
    X += 0.05 * (rs.randn(rows, F) + 1j * rs.randn(rows, F))
    X *= scale
    return X.real.astype(np.float32), X.imag.astype(np.float32)


def rel_err(y, ref):
    """max |y - ref| / max |ref| over BOTH parts of a case: y, ref = (re, im) tuples.  NaNs must sit in the same places and are left out."""
    yr, yi = (np.asarray(v, np.float64) for v in y)
    rr, ri = (np.asarray(v, np.float64) for v in ref)
    assert yr.shape == rr.shape and yi.shape == ri.shape, (yr.shape, rr.shape)
    assert np.array_equal(np.isnan(yr), np.isnan(rr)) and np.array_equal(np.isnan(yi), np.isnan(ri)), 'NaNs in other places'
    ok = ~np.isnan(rr)
    top = max(np.abs(rr[ok]).max(initial=0.0), np.abs(ri[ok]).max(initial=0.0))
    if top == 0.0:
        return float(max(np.abs(yr[ok]).max(initial=0.0), np.abs(yi[ok]).max(initial=0.0)))
    return float(max(np.abs(yr[ok] - rr[ok]).max(initial=0.0), np.abs(yi[ok] - ri[ok]).max(initial=0.0)) / top)
