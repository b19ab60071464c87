"""Record the reference's utils/silence.py on the cases of tests/test_silence_host.py and tests/test_gpu_silence.py (build container only).

    PSND_REFERENCE=/path/to/pytorch_sound python tools/gen_silence_golden.py      ->  tests/golden/silence.npz

The reference's module imports only numpy and itertools: it is loaded from its file, no stubs.  The file written holds data only: per
case the input row, (L, s, dB, keep_silence), the reference's silent and nonsilent ranges, and the lengths and concatenated samples of the
chunks of split_on_silence.  Before writing, every case is checked in float64 (tests/silence_ref.py, math.fsum): every window holds a
non-finite sample or its energy is at least 1e-3 theta away from theta (theta = 0: all zeros, or clearly more), so the reference's float32
dot products and float64 sums cannot decide differently; the smallest margin is stored as `min_margin`.
"""
import importlib.util
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get('PSND_REFERENCE', '/root/reference')
OUT = os.path.join(ROOT, 'tests', 'golden', 'silence.npz')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import silence_ref as S  # noqa: E402

INF = math.inf
KEEP = 5


def cases():
    """[(name, build(seed) -> row, L, s, dB)]: T in {1, 1023, 1024, 1025, 4101, 6000}, L in {1, 2, 1023, 1024, 1025, 2051, T, T + 1}, s in
    {1, 2, L, L + 1, 3L, > T}, last start on and off the grid, silence at the start and at the end, none at all, all of it, -inf dB on
    exact zeros, one NaN and one Inf sample"""
    g, rs = S.gated, S.random_spans
    out = [
        ('t1_zero', lambda k: np.zeros(1, np.float32), 1, 1, -40.0),
        ('t1_L2', lambda k: g(k, 1, []), 2, 1, -40.0),
        ('t1023_L1', lambda k: g(k, 1023, rs(k, 1023, 40)), 1, 1, -40.0),
        ('t1023_L2_s2_offgrid', lambda k: g(k, 1023, [(0, 31)] + rs(k, 1023, 30)), 2, 2, -40.0),
        ('t1024_L2_s2_ongrid', lambda k: g(k, 1024, rs(k, 1024, 30) + [(1001, 1024)]), 2, 2, -40.0),
        ('t1024_LT_all', lambda k: g(k, 1024, [(0, 1024)]), 1024, 1, -50.0),
        ('t1024_LT1', lambda k: g(k, 1024, [(0, 1024)]), 1025, 1, -50.0),
        ('t1025_L1023', lambda k: g(k, 1025, [(0, 1024)]), 1023, 1, -30.0),
        ('t1025_L1024_s3L', lambda k: g(k, 1025, [(1, 1025)]), 1024, 3072, -30.0),
        ('t1025_L2_zeros', lambda k: g(k, 1025, rs(k, 1025, 20, 6), 'zero'), 2, 1, -INF),
        ('t4101_L1025_start', lambda k: g(k, 4101, [(0, 1500), (2040, 3300)]), 1025, 1, -30.0),
        ('t4101_L2051_end', lambda k: g(k, 4101, [(1900 + k, 4101)]), 2051, 1, -30.0),
        ('t4101_L100_sL', lambda k: g(k, 4101, rs(k, 4101, 100, 6) + [(3900, 4101)]), 100, 100, -40.0),
        ('t4101_L100_sL1', lambda k: g(k, 4101, [(0, 333)] + rs(k, 4101, 100, 6)), 100, 101, -40.0),
        ('t4101_L50_s3L', lambda k: g(k, 4101, [(100, 900), (1500, 1580), (2000, 2700)]), 50, 150, -40.0),
        ('t6000_L1024_none', lambda k: g(k, 6000, []), 1024, 2, -20.0),
        ('t6000_L1023_sbig', lambda k: g(k, 6000, [(0, 1100), (4900, 6000)]), 1023, 7000, -30.0),
        ('t6000_L64_zeros', lambda k: g(k, 6000, rs(k, 6000, 64, 12) + [(5900, 6000)], 'zero'), 64, 1, -INF),
        ('t6000_L64_nonfinite', _nonfinite, 64, 1, -40.0),
        ('t6000_LT_zero', lambda k: np.zeros(6000, np.float32), 6000, 1, -INF),
    ]
    return out


def _nonfinite(k):
    """a NaN in the middle of one long quiet span, an Inf in the middle of another: each splits its silence in two, and the windows next to
    them stay silent"""
    x = S.gated(k, 6000, [(500, 1500), (3000, 4200)])
    x[1000] = np.nan
    x[3600] = np.inf
    return x


def main():
    spec = importlib.util.spec_from_file_location('ref_silence', os.path.join(REF, 'pytorch_sound', 'utils', 'silence.py'))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    data, names, least = {}, [], math.inf
    for name, build, L, s, db in cases():
        x = S.with_margin(build, L, s, db)
        m = S.assert_margin(x, L, s, db)
        if S.theta_of(L, db) > 0:
            least = min(least, m)
        with np.errstate(all='ignore'):
            silent = ref.detect_silence(x, L, db, s)
            nonsilent = ref.detect_nonsilent(x, L, db, s)
            chunks = ref.split_on_silence(x, L, db, KEEP, s)
        assert silent == S.detect_silence(x, L, db, s), name          # the yardstick agrees with the reference where the margin holds
        names.append(name)
        data[name + '.x'] = x
        data[name + '.params'] = np.array([L, s, db, KEEP], dtype=np.float64)
        data[name + '.silent'] = np.array(silent, dtype=np.int64).reshape(-1, 2)
        data[name + '.nonsilent'] = np.array(nonsilent, dtype=np.int64).reshape(-1, 2)
        data[name + '.chunk_len'] = np.array([len(c) for c in chunks], dtype=np.int64)
        data[name + '.chunks'] = np.concatenate(chunks).astype(np.float32) if chunks else np.zeros(0, np.float32)
        print('%-24s T=%5d L=%5d s=%5d dB=%6s  silent=%3d nonsilent=%3d margin=%.3g' % (name, x.size, L, s, db, len(silent), len(nonsilent), m))
    data['names'] = np.array(names)
    data['min_margin'] = np.array(least)
    np.savez_compressed(OUT, **data)
    print('%s: %d cases, %d bytes, smallest margin %.3g' % (OUT, len(names), os.path.getsize(OUT), least))
    assert os.path.getsize(OUT) < 256 * 1024


if __name__ == '__main__':
    main()
