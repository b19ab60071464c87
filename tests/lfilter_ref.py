"""Yardstick and bound of the recursive-filter tests (test infrastructure, never imported by the product).

Yardstick: scipy.signal.lfilter on the float64 copy of the float32 input - the function the reference itself calls; mirrored in time as
flip(lfilter(b, a, flip(g))).

Bound per element:  |got - y64| <= 2^-23 |y64[t]| + 2^-28 max|y64|.
  first term: the output is the float32 rounding of a float64 trajectory, half an ulp, doubled for slack;
  second term: the float64 reassociation of the scan.  A float64 numpy emulation of the chunk / level scheme of psnd_lfilter.hip against the
  sequential recurrence gave 3.2e-10 of max|y| at pole radius 0.998 (low-pass 20 Hz / 44.1 kHz, T = 40 000), 5.1e-12 at 0.990 and 4e-16 at
  0.97; 2^-28 = 3.7e-9 is ten times the worst of those.  The test filters stay at radius <= 0.998, so that the yardstick's own arithmetic
  stays inside the bound.
"""
import math

import numpy as np
from scipy import signal


def cookbook(kind, f, fs=44100, q=0.707):
    w0 = 2 * math.pi * f / fs
    c, alpha = math.cos(w0), math.sin(w0) / (2 * q)
    b = [(1 - c) / 2, 1 - c, (1 - c) / 2] if kind == 'low' else [(1 + c) / 2, -(1 + c), (1 + c) / 2]
    return b, [1 + alpha, -2 * c, 1 - alpha]


FILTERS = {
    'pole+0.97': ([1.0], [1.0, -0.97]),
    'pole-0.97': ([1.0], [1.0, 0.97]),
    'fir': ([1.0, -0.97], [1.0]),
    'lowpass100': cookbook('low', 100),
    'lowpass20': cookbook('low', 20),
    'highpass80': cookbook('high', 80),
    'integrator': ([1.0], [1.0, -1.0]),
}


def reference(x32, b, a, reverse=False):
    """float64 yardstick along the last axis of a float32 array"""
    x = np.asarray(x32, dtype=np.float32).astype(np.float64)
    if x.shape[-1] == 0:
        return x
    if reverse:
        return signal.lfilter(b, a, x[..., ::-1], axis=-1)[..., ::-1]
    return signal.lfilter(b, a, x, axis=-1)


def bound(y64):
    y64 = np.asarray(y64, dtype=np.float64)
    peak = np.abs(y64).max(axis=-1, keepdims=True) if y64.size else 0.0          # per row: the rows are independent signals
    return 2.0 ** -23 * np.abs(y64) + 2.0 ** -28 * peak


def excess(got, y64, scale=1.0):
    """largest |got - y64| / bound over the elements (<= 1 passes); `scale` widens the bound where a test states so"""
    got = np.asarray(got, dtype=np.float64)
    if got.size == 0:
        return 0.0
    bd = scale * bound(y64)
    err = np.abs(got - y64)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(bd, 1e-300))))


def signal_rows(seed, N, T):
    g = np.random.RandomState(seed)
    return (0.3 * g.randn(N, T)).astype(np.float32)
