"""psnd_loudness.hip on the GPU against the sequential yardstick tests/loudness_ref.py on the same fp32 samples: every seam of the scan at
sr = 8000 (B = 3200, H = 800 does not divide the span), batches and layouts, reproducibility and memory hygiene, the plain levels, the
gain, utils.sound.normalize and graph capture.

Tolerances.  lufs: 1e-4 LU - the fp64 arithmetic leaves errors near 1e-12, rounding the result to fp32 at |L| < 128 costs at most 3.8e-6,
the bound leaves a factor of 10 over that.  blocks: relative 1e-6 (half an fp32 ulp is 6e-8).  The inputs keep every z[j] at a relative
distance > 1e-6 from both gates; that condition is asserted on the yardstick in tests/test_loudness_host.py, on the CPU."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as R  # noqa: E402
import poison as P  # noqa: E402

pytestmark = pytest.mark.gpu

LUFS_TOL, BLOCK_RTOL = 1e-4, 1e-6


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _U():
    from pytorch_sound_amd.utils import sound
    return sound


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def reference(name, sr, T, C):
    """(samples, Reading) of a case, computed once"""
    x = R.case_input(name, sr, T, C)
    return x, R.measure(x, sr)


def _check(lufs, blocks, ref, what):
    lufs = float(lufs)
    print('%s: %.6f LUFS, yardstick %.6f, %d blocks' % (what, lufs, ref.lufs, len(ref.z)))
    if math.isinf(ref.lufs):
        assert lufs == ref.lufs, what
    else:
        assert abs(lufs - ref.lufs) <= LUFS_TOL, what
    if blocks is not None:
        b = blocks.double().cpu().numpy()
        J = len(ref.z)
        assert b.shape[0] >= J and not b[J:].any(), what
        if J:
            err = float(np.max(np.abs(b[:J] - ref.z) / ref.z))
            print('    blocks: largest relative error %.3g' % err)
            assert err <= BLOCK_RTOL, what


def test_the_library_reports_the_span_the_cases_are_built_on():
    assert _K().loudness_span() == R.SPAN


@pytest.mark.parametrize('name,sr,T,C', R.cases())
def test_accuracy_against_the_yardstick(name, sr, T, C):
    K = _K()
    x, ref = reference(name, sr, T, C)
    lufs, blocks = K.loudness(_dev(x), sr, channels=C, return_blocks=True)
    assert lufs.shape == () and lufs.dtype == torch.float32 and blocks.shape == (len(ref.z),)
    _check(lufs, blocks, ref, '%s sr=%d T=%s C=%s' % (name, sr, T, C))


def test_thirty_second_rows():
    K = _K()
    sr, T = 22050, 30 * 22050
    x = np.stack([R.gated_noise(40 + n, T, sr) * (0.5 ** n) for n in range(4)])
    lufs, blocks = K.loudness(_dev(x), sr, return_blocks=True)
    assert lufs.shape == (4,) and blocks.shape == (4, R.n_blocks(T, *R.block(sr)))
    for n in range(4):
        ref = R.measure(x[n], sr)
        assert ref.margin > R.MARGIN
        _check(lufs[n], blocks[n], ref, '30 s row %d' % n)


def test_given_weights():
    K = _K()
    for C, w in ((2, [0.25, 1.75]), (5, [0.5, 2.0, 1.0, 0.0, 1.25])):
        x, _ = reference('noise', 8000, {2: 2 * R.SPAN + 1, 5: R.SPAN + 1}[C], C)
        ref = R.measure(x, 8000, w)
        assert ref.margin > R.MARGIN
        lufs, blocks = K.loudness(_dev(x), 8000, channels=C, weights=w, return_blocks=True)
        _check(lufs, blocks, ref, 'C=%d weights=%r' % (C, w))
    with pytest.raises(K.PsndError):
        K.loudness(torch.zeros(6, 4000, device='cuda'), 8000, channels=6)


def test_a_row_alone_and_inside_a_batch_give_the_same_bits():
    K = _K()
    T = 2 * R.SPAN + 1
    a = reference('noise', 8000, T, None)[0]
    rows = np.stack([R.gated_noise(70, T, 8000), a, R.gated_noise(71, T, 8000)])
    one = K.loudness(_dev(a[None]), 8000, return_blocks=True)
    three = K.loudness(_dev(rows), 8000, return_blocks=True)
    assert P.same_bits(one[0][0], three[0][1]) and P.same_bits(one[1][0], three[1][1])


def test_ragged_rows_equal_the_rows_cut_out():
    K = _K()
    T = 3 * R.SPAN + 17
    lens = [T, 2 * R.SPAN + 1, R.SPAN, 3199, 0]
    rows = np.zeros((len(lens), T), dtype=np.float32)
    for n, ln in enumerate(lens):
        rows[n, :ln] = R.gated_noise(80 + n, T, 8000)[:ln]
    want = [K.loudness(_dev(rows[n:n + 1, :ln]), 8000, return_blocks=True) for n, ln in enumerate(lens)]
    garbage = rows.copy()
    for n, ln in enumerate(lens):
        garbage[n, ln:] = np.nan if n % 2 else 1e30                      # what lies behind a length changes nothing
    for batch in (rows, garbage):
        lufs, blocks = K.loudness(_dev(batch), 8000, lengths=torch.tensor(lens), return_blocks=True)
        for n, ln in enumerate(lens):
            J = R.n_blocks(ln, 3200, 800)
            assert P.same_bits(lufs[n], want[n][0][0]), n
            assert P.same_bits(blocks[n, :J], want[n][1][0]) and not bool(blocks[n, J:].any()), n
    assert float(lufs[3]) == -math.inf and float(lufs[4]) == -math.inf
    for kind in ('rms', 'peak'):
        got = K.level(_dev(garbage), kind, lengths=lens)
        for n, ln in enumerate(lens):
            assert P.same_bits(got[n], K.level(_dev(rows[n:n + 1, :ln]), kind)[0]), (kind, n)


def test_a_non_finite_sample_reads_nan_and_leaves_its_neighbours():
    K = _K()
    T = R.SPAN + 1
    rows = np.stack([R.gated_noise(90 + n, T, 8000) for n in range(3)])
    base = K.loudness(_dev(rows), 8000, return_blocks=True)
    for bad, at in ((np.nan, 5000), (np.inf, T - 1), (-np.inf, 0)):        # T - 1: behind the last complete block
        r = rows.copy()
        r[1, at] = bad
        lufs, blocks = K.loudness(_dev(r), 8000, return_blocks=True)
        assert math.isnan(float(lufs[1])) and bool(torch.isnan(blocks[1]).all())
        for n in (0, 2):
            assert P.same_bits(lufs[n], base[0][n]) and P.same_bits(blocks[n], base[1][n])
        for kind in ('rms', 'peak'):
            lv, g = K.level_gain(_dev(r), kind, -20.0)
            assert math.isnan(float(lv[1])) and float(g[1]) == 1.0 and math.isfinite(float(lv[0]))
        assert float(K.loudness_gain(_dev(r), 8000, -23.0)[1][1]) == 1.0


def test_layouts_and_dtypes():
    K, U = _K(), _U()
    T = 2 * R.SPAN + 1
    x, ref = reference('noise', 8000, T, None)
    want = K.loudness(_dev(x), 8000, return_blocks=True)
    # a view that starts 4 bytes off a 16-byte boundary, walked where it lies
    flat = torch.zeros(T + 8, device='cuda')
    view = flat[1:1 + T]
    view.copy_(_dev(x))
    assert view.data_ptr() % 16 == 4 and K._meter_rows(view, None, 'test')[0].data_ptr() == view.data_ptr()
    got = K.loudness(view, 8000, return_blocks=True)
    assert P.same_bits(got[0], want[0]) and P.same_bits(got[1], want[1])
    for kind in ('rms', 'peak'):
        assert P.same_bits(K.level(view, kind), K.level(_dev(x), kind))
    y = U.normalize(view, 8000, -23.0)
    assert P.same_bits(y, U.normalize(_dev(x), 8000, -23.0))
    # the same on a batch cut out of a wider one (x[..., 1:]) and on a transposed one
    wide = torch.zeros(3, T + 1, device='cuda')
    wide[:, 1:] = _dev(x)
    got = K.loudness(wide[..., 1:], 8000)
    assert got.shape == (3,) and all(P.same_bits(got[n], want[0]) for n in range(3))
    tr = _dev(np.stack([x, 0.5 * x])).t().contiguous().t()
    assert not tr.is_contiguous()
    got = K.loudness(tr, 8000)
    assert P.same_bits(got[0], want[0]) and abs(float(got[0] - got[1]) - 20.0 * math.log10(2.0)) <= 1e-4
    # other float dtypes are cast in; a waveform comes back as it went in
    assert P.same_bits(K.loudness(_dev(x).double(), 8000), want[0])
    xb = _dev(x).bfloat16()
    assert P.same_bits(K.loudness(xb, 8000), K.loudness(xb.float(), 8000))
    for t in (_dev(x).double(), xb, _dev(x).half()):
        y = U.normalize(t, 8000, -23.0)
        assert y.dtype == t.dtype and y.shape == t.shape and y.device == t.device
    # leading shapes
    got = K.loudness(_dev(np.stack([x, x]).reshape(2, 1, T)), 8000)
    assert got.shape == (2, 1)
    got = K.loudness(_dev(np.stack([x, x]).reshape(1, 2, T)), 8000, channels=2)
    assert got.shape == (1,)
    assert K.loudness(torch.zeros(0, 4000, device='cuda'), 8000).shape == (0,)


def test_two_runs_and_poisoned_memory_give_the_same_bits():
    K, U = _K(), _U()
    x = _dev(np.stack([reference('noise', 8000, 3 * R.SPAN + 17, None)[0], reference('loud_quiet', 8000, 3 * R.SPAN + 17, None)[0]]))
    lens = torch.tensor([3 * R.SPAN + 17, R.SPAN + 5], device='cuda')

    def run():
        lufs, gain, blocks = K.loudness_gain(x, 8000, -23.0, lens, return_blocks=True)
        return [lufs, gain, blocks, K.level_gain(x, 'rms', -20.0, lens), K.level_gain(x, 'peak', -1.0, lens), U.normalize(x, 8000, -23.0)]

    a, b = P.to_cpu(run()), P.to_cpu(run())
    assert not P.differences([a, b], (0, 1))
    P.assert_same_bits(run)


def test_nothing_outside_the_outputs_is_written():
    K = _K()
    from pytorch_sound_amd._lib import lib, on
    N, C, T, sr = 2, 2, R.SPAN + 1, 8000
    B, H = K.loudness_block(sr)
    J = K.loudness_blocks(T, B, H)
    x = _dev(np.stack([R.gated_noise(60 + n, T, sr, C) for n in range(N)]))
    (b1, a1), (b2, a2) = K.k_weighting(sr)
    nbytes = int(lib().psnd_loudness_scratch_bytes(N, C, T, B, H))
    guard = 64
    outs = {}
    for fill in (0.0, math.nan):
        scratch = torch.full((nbytes + 2 * guard * 4,), 0x5A, dtype=torch.uint8, device='cuda')
        f = torch.full((3 * guard + 2 * N + N * J + guard,), fill, device='cuda')
        before = f.clone()
        lufs, gain, blocks = f[guard:guard + N], f[2 * guard + N:2 * guard + 2 * N], f[3 * guard + 2 * N:3 * guard + 2 * N + N * J]
        with on(x.device) as hip:
            hip.psnd_loudness(x, N, C, T, None, b1[0], b1[1], b1[2], a1[1], a1[2], b2[0], b2[1], b2[2], a2[1], a2[2], B, H, None, -23.0,
                              scratch[guard * 4:guard * 4 + nbytes], lufs, blocks, gain)
        torch.cuda.synchronize()
        assert bool((scratch[:guard * 4] == 0x5A).all()) and bool((scratch[guard * 4 + nbytes:] == 0x5A).all())
        written = torch.zeros_like(f, dtype=torch.bool)
        for lo, n in ((guard, N), (2 * guard + N, N), (3 * guard + 2 * N, N * J)):
            written[lo:lo + n] = True
        assert P.same_bits(f[~written], before[~written])
        assert bool(torch.isfinite(f[written]).all())
        outs[fill == 0.0] = f[written].clone()
    assert P.same_bits(outs[True], outs[False])
    want = K.loudness(x, sr, channels=C)
    assert P.same_bits(outs[True][:N], want)


def test_levels_against_numpy():
    K = _K()
    rows = np.stack([R.gated_noise(20 + n, 5 * 4096 + 3, 8000) * (0.3 ** n) for n in range(3)] + [np.zeros(5 * 4096 + 3, dtype=np.float32)])
    for kind, ref in (('rms', R.rms_db), ('peak', R.peak_db)):
        got = K.level(_dev(rows), kind)
        assert got.dtype == torch.float32 and got.shape == (4,)
        for n in range(3):
            print('%s row %d: %.6f dB, numpy %.6f' % (kind, n, float(got[n]), ref(rows[n])))
            assert abs(float(got[n]) - ref(rows[n])) <= 1e-4
        assert float(got[3]) == -math.inf
        two = K.level(_dev(rows[:2][None]), kind, channels=2)               # one programme of two channels
        assert two.shape == (1,) and abs(float(two[0]) - ref(rows[:2])) <= 1e-4
    assert K.level(torch.zeros(2, 0, device='cuda'), 'rms').tolist() == [-math.inf, -math.inf]
    with pytest.raises(ValueError):
        K.level(_dev(rows), 'lufs')


def test_apply_gain_in_place_and_out_of_place():
    K = _K()
    T = 4 * 1024 + 3
    x = np.stack([R.gated_noise(30 + n, T, 8000) for n in range(4)])
    g = np.asarray([2.0, 0.5, 1.0, -3.0], dtype=np.float32)
    lens = [T, 1001, 0, T - 1]
    want = x * g[:, None]
    for n, ln in enumerate(lens):
        want[n, ln:] = x[n, ln:]
    d = _dev(x)
    y = K.apply_gain(d, _dev(g), lengths=lens)
    assert y.data_ptr() != d.data_ptr() and np.array_equal(y.cpu().numpy(), want) and np.array_equal(d.cpu().numpy(), x)
    same = K.apply_gain(d, _dev(g), lengths=lens, out=d)
    assert same is d and np.array_equal(d.cpu().numpy(), want)
    pair = K.apply_gain(_dev(x.reshape(2, 2, T)), _dev(g[:2]), channels=2)     # one gain per programme of two channels
    assert np.array_equal(pair.cpu().numpy(), x.reshape(2, 2, T) * g[:2, None, None])
    with pytest.raises(K.PsndError):
        K.apply_gain(d, _dev(g[:3]))


@pytest.mark.parametrize('kind,target', [('ebu', -23.0), ('ebu', -16.0), ('rms', -20.0), ('peak', -1.0)])
def test_normalize_reaches_the_target(kind, target):
    K, U = _K(), _U()
    sr, T = 8000, R.SPAN + 1
    x = np.stack([R.gated_noise(50, T, sr), np.zeros(T, dtype=np.float32), 4.0 * R.gated_noise(51, T, sr)])
    y = U.normalize(_dev(x), sr, target, kind)
    assert y.dtype == torch.float32 and y.shape == x.shape and y.is_cuda
    out = y.cpu().numpy()
    assert np.array_equal(out[1], x[1])                                  # a silent row comes back bit-identical
    measure = {'ebu': lambda v: R.measure(v, sr).lufs, 'rms': R.rms_db, 'peak': R.peak_db}[kind]
    for n in (0, 2):
        got = measure(out[n])
        print('%s row %d: %.5f, target %.1f' % (kind, n, got, target))
        assert abs(got - target) <= 1e-3
    again = K.loudness(y, sr) if kind == 'ebu' else K.level(y, kind)
    assert abs(float(again[0]) - target) <= 1e-3 and abs(float(again[2]) - target) <= 1e-3
    short = _dev(x[:1, :3199])                                           # one sample short of a block
    if kind == 'ebu':
        assert P.same_bits(U.normalize(short, sr, target, kind), short)
    from pytorch_sound_amd.models.sound import LoudnessNorm
    mod = LoudnessNorm(sr, target, kind).cuda()
    assert P.same_bits(mod(_dev(x)), y) and P.same_bits(mod(_dev(x)[:, None, :]), y[:, None, :])
    grad = _dev(x).requires_grad_(True)
    assert not U.normalize(grad, sr, target, kind).requires_grad


def test_graph_capture_replays_on_new_input():
    K, U = _K(), _U()
    sr, T = 8000, 2 * R.SPAN + 1
    a = np.stack([R.gated_noise(100, T, sr), R.gated_noise(101, T, sr)])
    b = np.stack([0.1 * R.gated_noise(102, T, sr), np.zeros(T, dtype=np.float32)])
    buf = _dev(a)

    def run():
        return K.loudness(buf, sr, return_blocks=True), U.normalize(buf, sr, -23.0), U.normalize(buf, sr, -3.0, 'peak')

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                            # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for data in (a, b):
        buf.copy_(_dev(data))
        graph.replay()
        torch.cuda.synchronize()
        got = P.to_cpu(captured)
        assert not P.differences([P.to_cpu(run()), got], (0, 1))
    assert float(got[0][0][1]) == -math.inf and np.array_equal(got[1][1].numpy(), b[1])
