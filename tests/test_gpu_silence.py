"""psnd_silence.hip on the GPU: the recorded reference results (tests/golden/silence.npz), many short ranges across every seam of the range
kernel, the loud-then-quiet accuracy row, ragged rows, layouts and dtypes, the public functions of utils.silence, memory hygiene and graph
capture.  All comparisons are exact equality of integers: the inputs carry a margin (tests/silence_ref.py), so there is no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import silence_ref as S  # noqa: E402
import poison as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _M():
    from pytorch_sound_amd.utils import silence
    return silence


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def G(golden):
    return golden('silence')


def _case(G, name):
    L, s, db, keep = G[name + '.params'].tolist()
    return G[name + '.x'], int(L), int(s), db, int(keep)


def _unpack(count, ranges):
    """(count, ranges) of the device -> per-row lists, with the layout checked: -1 behind every row's ranges"""
    count, ranges = count.cpu().numpy(), ranges.cpu().numpy()
    assert count.dtype == np.int32 and ranges.dtype == np.int64 and ranges.shape[0] == count.shape[0] and ranges.shape[2] == 2
    out = []
    for c, r in zip(count.tolist(), ranges):
        assert 0 <= c <= r.shape[0] and (r[c:] == -1).all() and (r[:c] >= 0).all()
        out.append(r[:c].tolist())
    return out


def _names():
    return [str(n) for n in np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'silence.npz'))['names']]


@pytest.mark.parametrize('name', _names())
def test_golden_cases(G, name):
    K = _K()
    x, L, s, db, _ = _case(G, name)
    count, ranges = K.silence_ranges(_dev(x), L, db, s)
    assert ranges.shape == (1, S.cap(x.size, L), 2)
    assert _unpack(count, ranges) == [G[name + '.silent'].tolist()]


def test_many_short_ranges_cross_every_seam():
    """L = 3, s = 1, a burst every 9 samples of 5000: one range per gap - the heads fall on every lane, wave and chunk seam of the range kernel
    (16 starts per lane, 4096 per chunk), and the ranges fill less than the cap, so the -1 fill is there to check"""
    K = _K()
    x = S.bursts()
    S.assert_margin(x, 3, 1, -40.0)
    want = S.detect_silence(x, 3, -40.0, 1)
    count, ranges = K.silence_ranges(_dev(x), 3, -40.0, 1)
    assert 500 < len(want) < S.cap(x.size, 3) == ranges.shape[1]
    assert _unpack(count, ranges) == [want]


def test_quiet_windows_behind_a_loud_passage():
    """the row on which differences of a row-long float64 prefix decide wrongly (asserted in tests/test_silence_host.py)"""
    K = _K()
    x, db = S.loud_then_quiet()
    S.assert_margin(x, S.ACC_L, 1, db, least=1e-6)
    count, ranges = K.silence_ranges(_dev(x), S.ACC_L, db, 1)
    assert _unpack(count, ranges) == [S.detect_silence(x, S.ACC_L, db, 1)]


@pytest.mark.parametrize('L,lengths', [(100, (4101, 1500, 0)), (1025, (1024, 1025, 1026))])
def test_ragged_rows_equal_the_rows_one_at_a_time(L, lengths):
    K = _K()
    T, s, db = 4101, 3, -40.0
    rows = [S.with_margin(lambda k: S.gated(k + 10 * n, T, [(0, 1026)] + S.random_spans(k + n, T, L, 4)), L, s, db, also=(lengths[n],))
            for n in range(3)]
    x = _dev(np.stack(rows))
    for lens in (list(lengths), torch.tensor(lengths, device=DEV)):
        got = _unpack(*K.silence_ranges(x, L, db, s, lengths=lens))
        assert got == [S.detect_silence(rows[n][:lengths[n]], L, db, s) for n in range(3)]
        assert got == [_unpack(*K.silence_ranges(x[n, :lengths[n]], L, db, s))[0] for n in range(3)]
    assert got[0] or got[1]


def test_layouts_and_dtypes():
    K = _K()
    T, L, s, db = 4101, 64, 1, -40.0
    x = S.with_margin(lambda k: S.gated(k, T + 1, S.random_spans(k, T, L, 6)), L, s, db, also=(T,))
    S.assert_margin(x[1:], L, s, db)                    # s = 1: the windows of x[1:] are windows of x
    # a 1-D view whose base is 4 bytes off a 16-byte boundary
    big = _dev(x)
    view = big[1:]
    assert view.data_ptr() % 16 == 4
    assert _unpack(*K.silence_ranges(view, L, db, s)) == [S.detect_silence(x[1:], L, db, s)]
    # a non-contiguous view, and a leading shape
    two = np.stack([x[:T], x[:T][::-1]])
    S.assert_margin(two[1], L, s, db)
    want = [S.detect_silence(r, L, db, s) for r in two]
    inter = torch.empty(T, 2, device=DEV)
    inter.copy_(_dev(two).t())
    assert not inter.t().is_contiguous()
    assert _unpack(*K.silence_ranges(inter.t(), L, db, s)) == want
    count, ranges = K.silence_ranges(_dev(two).reshape(2, 1, T), L, db, s)
    assert count.shape == (2,) and _unpack(count, ranges) == want
    # fp16 / bf16: the fp32 result of the cast values (the quiet noise and the loud multiples of 1/256 are exact in both)
    for dt in (torch.float16, torch.bfloat16):
        h = _dev(x[:T]).to(dt)
        assert _unpack(*K.silence_ranges(h, L, db, s)) == _unpack(*K.silence_ranges(h.float(), L, db, s))
    assert _unpack(*K.silence_ranges(_dev(x[:T]).half(), L, db, s)) == [want[0]]
    with pytest.raises(K.PsndError):
        K.silence_ranges(_dev(x).double(), L, db, s)
    with pytest.raises(K.PsndError):
        K.silence_ranges(torch.zeros(64, dtype=torch.int32, device=DEV), L, db, s)
    assert K.silence_ranges(torch.zeros(2, 0, device=DEV), L, db, s)[0].tolist() == [0, 0]


def test_public_functions_on_hip_tensors(G):
    M = _M()
    for name in ('t4101_L100_sL', 't6000_L64_nonfinite', 't1024_LT_all', 't1_L2', 't4101_L1025_start'):
        x, L, s, db, keep = _case(G, name)
        d = _dev(x)
        assert M.detect_silence(d, L, db, s) == M.detect_silence(x, L, db, s) == G[name + '.silent'].tolist()
        assert M.detect_nonsilent(d, L, db, s) == M.detect_nonsilent(x, L, db, s) == G[name + '.nonsilent'].tolist()
        got, want = M.split_on_silence(d, L, db, keep, s), M.split_on_silence(x, L, db, keep, s)
        assert len(got) == len(want)
        for (a, _), c, w in zip(M.detect_nonsilent(x, L, db, s), got, want):
            assert c.data_ptr() == d.data_ptr() + 4 * max(0, a - keep)       # a view of the input
            assert np.array_equal(c.cpu().numpy(), w, equal_nan=True)
    x, L, s, db, _ = _case(G, 't4101_L100_sL')
    batch = np.stack([x, x[::-1]])
    S.assert_margin(batch[1][:3000], L, s, db)
    got = M.detect_nonsilent(_dev(batch), L, db, s, lengths=[4101, 3000])
    assert got == M.detect_nonsilent(batch, L, db, s, lengths=[4101, 3000]) == [S.detect_nonsilent(x, L, db, s), S.detect_nonsilent(batch[1][:3000], L, db, s)]
    assert float(M.rms(_dev(x))) == pytest.approx(float(M.rms(x)), rel=1e-5)


@pytest.mark.parametrize('L,s', [(64, 1), (2051, 3)])
def test_same_bits_on_poisoned_memory(L, s):
    """count, ranges and the scratch (prefixes, flags) come from torch.empty: every entry read must have been written by the call"""
    K = _K()
    T, db = 4101, -40.0
    rows = [S.with_margin(lambda k: S.gated(k + n, T, [(100, 2400)] + S.random_spans(k + n, T, 64, 5)), L, s, db, also=(1500,)) for n in range(2)]
    x = _dev(np.stack(rows))
    lengths = torch.tensor([T, 1500], device=DEV)

    def fn():
        return list(K.silence_ranges(x, L, db, s, lengths=lengths))

    first = P.assert_same_bits(fn)
    assert _unpack(*first) == [S.detect_silence(rows[0], L, db, s), S.detect_silence(rows[1][:1500], L, db, s)]


def test_graph_capture_replays_on_new_input(G):
    K = _K()
    a, L, s, db, _ = _case(G, 't6000_L64_nonfinite')
    b = _case(G, 't6000_L64_zeros')[0]
    S.assert_margin(b, L, s, db)
    buf = _dev(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        K.silence_ranges(buf, L, db, s)                 # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        count, ranges = K.silence_ranges(buf, L, db, s)
    graph.replay()
    torch.cuda.synchronize()
    assert _unpack(count, ranges) == [G['t6000_L64_nonfinite.silent'].tolist()]
    buf.copy_(_dev(b))
    graph.replay()
    torch.cuda.synchronize()
    want = S.detect_silence(b, L, db, s)
    assert want and want != G['t6000_L64_nonfinite.silent'].tolist()
    assert _unpack(count, ranges) == [want] == _unpack(*K.silence_ranges(buf, L, db, s))
