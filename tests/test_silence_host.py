"""utils.silence without a GPU: the alias import, the numpy / CPU-tensor restatement against the reference's recorded results
(tests/golden/silence.npz, tools/gen_silence_golden.py), batches with lengths, the edge cases of the definition, and the host side of the C
ABI (declared, exported, mirrored; bad arguments; psnd_silence_cap / psnd_silence_starts against the yardstick tests/silence_ref.py)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import silence_ref as S  # noqa: E402
from conftest import ROOT  # noqa: E402


@pytest.fixture(scope='module')
def G(golden):
    return golden('silence')


def _case(G, name):
    L, s, db, keep = G[name + '.params'].tolist()
    return G[name + '.x'], int(L), int(s), db, int(keep)


def _chunks(G, name):
    flat, out, at = G[name + '.chunks'], [], 0
    for n in G[name + '.chunk_len'].tolist():
        out.append(flat[at:at + n])
        at += n
    return out


def _M():
    from pytorch_sound_amd.utils import silence
    return silence


def test_alias_is_the_same_module():
    import pytorch_sound.utils.silence as a
    import pytorch_sound_amd.utils.silence as b
    assert a is b
    for name in ('rms', 'db_to_float', 'detect_silence', 'detect_nonsilent', 'split_on_silence'):
        assert callable(getattr(a, name))


def test_signatures_and_defaults_are_the_references():
    import inspect
    M = _M()
    want = {'detect_silence': [('min_silence_len', 1000), ('silence_thresh', -16), ('seek_step', 1)],
            'detect_nonsilent': [('min_silence_len', 1000), ('silence_thresh', -16), ('seek_step', 1)],
            'split_on_silence': [('min_silence_len', 1000), ('silence_thresh', -16), ('keep_silence', 100), ('seek_step', 1)]}
    for name, params in want.items():
        p = list(inspect.signature(getattr(M, name)).parameters.values())
        assert p[0].name == 'audio_segment' and [(q.name, q.default) for q in p[1:1 + len(params)]] == params, name
    assert M.db_to_float(-20) == pytest.approx(0.1) and M.db_to_float(-20, using_amplitude=False) == pytest.approx(0.01)
    x = np.array([3.0, 4.0], dtype=np.float32)
    assert M.rms(x) == pytest.approx(math.sqrt(12.5))
    r = M.rms(torch.from_numpy(x))
    assert isinstance(r, torch.Tensor) and r.dim() == 0 and float(r) == pytest.approx(math.sqrt(12.5))


def test_golden_margin_is_recorded(G):
    assert float(G['min_margin']) >= S.MARGIN
    assert len(G['names']) >= 20


@pytest.mark.parametrize('kind', ['numpy', 'cpu_tensor'])
def test_host_paths_equal_the_reference(G, kind):
    M = _M()
    for name in G['names'].tolist():
        x, L, s, db, keep = _case(G, name)
        a = x if kind == 'numpy' else torch.from_numpy(x.copy())
        assert M.detect_silence(a, L, db, s) == G[name + '.silent'].tolist(), name
        assert M.detect_nonsilent(a, L, db, s) == G[name + '.nonsilent'].tolist(), name
        got, want = M.split_on_silence(a, L, db, keep, s), _chunks(G, name)
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            g = g if kind == 'numpy' else g.numpy()
            assert np.array_equal(g, w, equal_nan=True), name
        assert all(type(v) is int for r in M.detect_silence(a, L, db, s) for v in r)


def test_chunks_are_views_of_the_input(G):
    M = _M()
    x, L, s, db, keep = _case(G, 't4101_L100_sL')
    for a in (x, torch.from_numpy(x.copy())):
        chunks = M.split_on_silence(a, L, db, keep, s)
        assert chunks
        for (b, _), c in zip(M.detect_nonsilent(a, L, db, s), chunks):
            if isinstance(a, np.ndarray):
                assert np.shares_memory(a, c)
            else:
                assert c.data_ptr() == a.data_ptr() + 4 * max(0, b - keep)


def test_yardstick_equals_the_reference_on_the_golden_cases(G):
    for name in G['names'].tolist():
        x, L, s, db, _ = _case(G, name)
        assert S.detect_silence(x, L, db, s) == G[name + '.silent'].tolist(), name
        assert S.detect_nonsilent(x, L, db, s) == G[name + '.nonsilent'].tolist(), name
        S.assert_margin(x, L, s, db)


def test_batch_with_lengths_equals_the_rows(G):
    M = _M()
    from pytorch_sound_amd import kernels
    L, s, db = 100, 7, -40.0
    T = 4101
    lengths = [T, 1500, 0]
    rows = [S.with_margin(lambda k: S.gated(k + 10 * n, T, S.random_spans(k + n, T, L, 5)), L, s, db, also=(lengths[n],)) for n in range(3)]
    batch = torch.from_numpy(np.stack(rows))
    for fn in (M.detect_silence, M.detect_nonsilent):
        got = fn(batch, L, db, s, lengths=lengths)
        assert got == [fn(rows[n][:lengths[n]], L, db, s) for n in range(3)]
        assert fn(np.stack(rows), L, db, s, lengths=lengths) == got
    assert got[2] == [[0, 0]] and M.detect_silence(batch, L, db, s, lengths=lengths)[2] == []
    chunks = M.split_on_silence(batch, L, db, 5, s, lengths=torch.tensor(lengths))
    for n in range(3):
        want = M.split_on_silence(rows[n][:lengths[n]], L, db, 5, s)
        assert len(chunks[n]) == len(want) and all(np.array_equal(c.numpy(), w) for c, w in zip(chunks[n], want))
    count, ranges = kernels.silence_ranges(batch, L, db, s, lengths=lengths)
    wc, wr = S.packed(rows, L, db, s, lengths)
    assert count.dtype == torch.int32 and ranges.dtype == torch.int64 and ranges.shape == (3, S.cap(T, L), 2)
    assert np.array_equal(count.numpy(), wc) and np.array_equal(ranges.numpy(), wr)


def test_edges_of_the_definition():
    M = _M()
    loud = S.gated(0, 50, [])
    assert M.detect_silence(loud, 51, -40.0) == [] and M.detect_nonsilent(loud, 51, -40.0) == [[0, 50]]          # T < L
    quiet = np.zeros(50, np.float32)
    assert M.detect_silence(quiet, 51, -40.0) == [] and M.detect_nonsilent(quiet, 51, -40.0) == [[0, 50]]
    assert M.detect_silence(quiet, 7, -40.0, 3) == [[0, 50]] and M.detect_nonsilent(quiet, 7, -40.0, 3) == []    # wholly silent
    assert M.split_on_silence(quiet, 7, -40.0) == []
    x = S.gated(1, 60, [(0, 20)])                                     # silence at the start: the [0, 0] gap in front of it is dropped
    assert M.detect_silence(x, 10, -40.0) == [[0, 20]] and M.detect_nonsilent(x, 10, -40.0) == [[20, 60]]
    x = S.gated(1, 60, [(45, 60)])                                    # and at the end: no empty gap behind it
    assert M.detect_silence(x, 10, -40.0) == [[45, 60]] and M.detect_nonsilent(x, 10, -40.0) == [[0, 45]]
    # s > L: grid neighbours merge across the gap between them; a start that is neither a neighbour nor within L opens a range
    x = S.gated(2, 100, [(0, 100)])
    x[31] = 0.5                                                       # starts 0, 10, 20, 30, ...: the windows at 30 = [30, 33) is loud
    assert M.detect_silence(x, 3, -40.0, 10) == [[0, 23], [40, 93], [97, 100]]
    # -inf dB: exact zeros only
    x = S.gated(3, 40, [(10, 20)], 'zero')
    x[25:30] = 2.0 ** -16                                             # the smallest non-zero sample the margin of silence_ref.py admits
    assert M.detect_silence(x, 4, -math.inf) == [[10, 20]]
    # a NaN is not silent and touches no window that does not hold it
    x = np.zeros(30, np.float32)
    x[12] = np.nan
    assert M.detect_silence(x, 5, -40.0) == [[0, 12], [13, 30]]
    x[12] = np.inf
    assert M.detect_silence(torch.from_numpy(x), 5, -40.0) == [[0, 12], [13, 30]]
    for bad in ((0, 1), (5, 0), (2.5, 1)):
        with pytest.raises(ValueError):
            M.detect_silence(x, bad[0], -40.0, bad[1])
    from pytorch_sound_amd import kernels
    with pytest.raises(kernels.PsndError):
        kernels.silence_ranges(torch.zeros(8, dtype=torch.int16), 2, -40.0)


def test_a_global_prefix_gets_the_accuracy_case_wrong():
    """the loud-then-quiet row of the GPU accuracy case keeps its teeth: differences of one row-long float64 prefix sum decide at least one
    window differently from the exact energies, the block-local restatement does not"""
    from pytorch_sound_amd import kernels
    x, db = S.loud_then_quiet()
    L = S.ACC_L
    S.assert_margin(x, L, 1, db, least=1e-6)
    th = S.theta_of(L, db)
    assert th == kernels.silence_theta(L, db)
    exact = np.array([E <= th for _, E, _ in S.energies(x, L, 1)])
    assert exact[len(x) // 2:].any() and not exact[len(x) // 2:].all()
    wrong = int(((S.global_prefix_energies(x, L) <= th) != exact).sum())
    print('global float64 prefix: %d of %d decisions differ from the exact ones' % (wrong, exact.size))
    assert wrong >= 1
    E, bad = kernels.silence_energies(x, L, kernels.silence_starts(len(x), L, 1))
    assert np.array_equal(E <= th, exact) and not bad.any()
    assert kernels.silence_ranges_host(x, L, 1, th).tolist() == S.detect_silence(x, L, db, 1)


def test_random_families_equal_the_yardstick():
    from pytorch_sound_amd import kernels
    r = np.random.RandomState(7)
    for k in range(40):
        T = int(r.randint(1, 3000))
        L = int(r.randint(1, 400))
        s = int(r.randint(1, 500))
        db = float(r.choice([-40.0, -30.0, -math.inf]))
        quiet = 'zero' if db == -math.inf else 'noise'
        x = S.with_margin(lambda seed: S.gated(seed + k, T, S.random_spans(seed + k, T, L, 5), quiet), L, s, db)
        got = kernels.silence_ranges_host(x, L, s, S.theta_of(L, db)).tolist()
        assert got == S.detect_silence(x, L, db, s), (T, L, s, db)
        assert len(got) <= S.cap(T, L)


# ---- the C ABI, host side -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.lib()


NAMES = ('psnd_silence_cap', 'psnd_silence_starts', 'psnd_silence_scratch_bytes', 'psnd_silence_ranges')


def test_entries_are_declared_exported_and_mirrored(lib):
    from pytorch_sound_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'psnd.h')).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + '(' in header and hasattr(h, n) and n in _lib.SIGNATURES, n
    assert '#define PSND_SILENCE_BLOCK 1024' in header
    assert len(_lib.SIGNATURES['psnd_silence_ranges'][1]) == 12
    assert lib.psnd_version() >= 146


def test_bad_arguments_return_e_arg(lib):
    buf = (ctypes.c_double * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    ok = dict(x=p, N=1, T=100, lengths=None, L=10, s=1, theta=0.1, scratch=p, count=p, ranges=p, cap=S.cap(100, 10), stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.psnd_silence_ranges(*[a[k] for k in ok])

    assert call(L=0) == -1 and call(L=-3) == -1
    assert call(s=0) == -1
    assert b'silence' in lib.psnd_last_error()
    assert call(cap=S.cap(100, 10) - 1) == -1
    assert call(theta=math.nan) == -1
    assert call(x=None) == -1 and call(count=None) == -1 and call(ranges=None) == -1 and call(scratch=None) == -1
    assert call(N=-1) == -1 and call(T=-1) == -1
    assert call(N=0) == 0 and call(T=0, cap=0) == 0                   # nothing to do, nothing launched
    assert call(N=0, x=None, count=None, ranges=None, scratch=None) == 0


def test_cap_starts_and_scratch_against_the_yardstick(lib):
    grid_T = (0, 1, 2, 5, 10, 11, 1023, 1024, 1025, 4101)
    grid_L = (1, 2, 3, 5, 10, 11, 1024, 1025, 5000)
    grid_s = (1, 2, 3, 7, 10, 1024, 6000)
    for T in grid_T:
        for L in grid_L + (T, T + 1):
            if L < 1:
                continue
            assert lib.psnd_silence_cap(T, L) == S.cap(T, L), (T, L)
            for s in grid_s + (T + 1,):
                n = len(S.starts(T, L, s))
                assert lib.psnd_silence_starts(T, L, s) == n, (T, L, s)
                if T > 0:
                    assert lib.psnd_silence_scratch_bytes(3, T, L, s) >= 3 * (12 * T + n)
    assert lib.psnd_silence_cap(10, 0) == 0 and lib.psnd_silence_starts(10, 0, 1) == 0 and lib.psnd_silence_starts(10, 1, 0) == 0
    assert lib.psnd_silence_scratch_bytes(0, 10, 1, 1) == 0
    # the cap is reached: L zeros, one loud sample, L zeros, ...
    from pytorch_sound_amd import kernels
    for T, L in ((20, 1), (23, 3), (24, 3)):
        x = np.zeros(T, np.float32)
        x[L::L + 1] = 0.5
        assert len(kernels.silence_ranges_host(x, L, 1, S.theta_of(L, -40.0))) == S.cap(T, L)
