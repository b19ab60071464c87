"""pytorch_sound.utils.sound on HIP tensors (psnd_lfilter.hip): the golden fixture of the reference, every seam of the scan (chunk, wave,
span, launch boundary) for both instances in both directions, shapes and dtypes, the gradient, graph capture, memory the path did not
write, library ops, and a NaN in the input.  Yardstick and bound: tests/lfilter_ref.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lfilter_ref as R  # noqa: E402
import poison as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SPAN = 8192
LENGTHS = (1, 2, 31, 32, 33, 2047, 2048, 2049, 8191, 8192, 8193, 3 * SPAN + 5)
BIG = 3 * SPAN + 5


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _snd():
    import pytorch_sound.utils.sound as m
    return m


@functools.lru_cache(maxsize=None)
def _rows(T, N=3):
    return R.signal_rows(1000 + T, N, T)


@functools.lru_cache(maxsize=None)
def _ref(name, T, reverse):
    return R.reference(_rows(T), *R.FILTERS[name], reverse)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _report(what, worst):
    print('%s: worst |error| / bound = %.3f' % (what, worst))


# ---- goldens ------------------------------------------------------------------------------------------------------------------------------
def test_golden_fixture_on_hip_tensors(golden):
    g = golden('utils_sound')
    x = _dev(g['x'])
    snd = _snd()
    for name, tag, coeff in (('preemphasis', '0p97', 0.97), ('inv_preemphasis', '0p97', 0.97), ('preemphasis', '0p5', 0.5),
                             ('inv_preemphasis', '0p5', 0.5)):
        got = getattr(snd, name)(x, coeff)
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == x.shape
        want = g['%s_%s' % (name, tag)].astype(np.float64)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        print('%s %s: max |error| / (2^-23 |golden|) = %.3f' % (name, tag, np.max(err / np.maximum(2.0 ** -23 * np.abs(want), 1e-300))))
        assert (err <= 2.0 ** -23 * np.abs(want)).all(), name            # within one float32 ulp of the golden


# ---- seams, both instances, both directions -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(R.FILTERS))
def test_seams_both_instances_both_directions(name):
    K = _K()
    b, a = R.FILTERS[name]
    assert K.lfilter_instance(b, a) == K.LFILTER_PARALLEL
    worst = {}
    for T in LENGTHS:
        x = _dev(_rows(T))
        assert T % 2 == 0 or x[1].data_ptr() % 16 != 0                   # an odd T puts rows 1 and 2 off a 16-byte boundary
        for reverse in (False, True):
            y64 = _ref(name, T, reverse)
            out = {}
            for inst in (K.LFILTER_PARALLEL, K.LFILTER_SEQ):
                out[inst] = K.lfilter(x, b, a, reverse=reverse, instance=inst).cpu().numpy()
                e = R.excess(out[inst], y64)
                worst[inst] = max(worst.get(inst, 0.0), e)
                assert e <= 1.0, (name, T, reverse, inst, e)
            d = np.abs(out[K.LFILTER_PARALLEL].astype(np.float64) - out[K.LFILTER_SEQ])
            assert (d <= 2 * R.bound(y64)).all(), (name, T, reverse)     # the two instances against each other: twice the bound
            if name == 'fir' or T <= 32:                                 # one chunk, or no state to carry: the same arithmetic
                assert np.array_equal(out[K.LFILTER_PARALLEL], out[K.LFILTER_SEQ]), (name, T, reverse)
    _report('%s parallel' % name, worst[K.LFILTER_PARALLEL])
    _report('%s sequential' % name, worst[K.LFILTER_SEQ])


def test_growing_filter_stays_on_the_parallel_instance():
    """a = [1, -1.001] at T = 8193: 1.001^8193 = 3.6e3, every power of the state matrix is finite"""
    K = _K()
    b, a = [1.0], [1.0, -1.001]
    assert K.lfilter_instance(b, a) == K.LFILTER_PARALLEL
    x = _rows(8193)
    for reverse in (False, True):
        y64 = R.reference(x, b, a, reverse)
        par = K.lfilter(_dev(x), b, a, reverse=reverse).cpu().numpy()
        seq = K.lfilter(_dev(x), b, a, reverse=reverse, instance=K.LFILTER_SEQ).cpu().numpy()
        _report('growing, reverse=%s' % reverse, max(R.excess(par, y64), R.excess(seq, y64)))
        assert R.excess(par, y64) <= 1.0 and R.excess(seq, y64) <= 1.0
        assert (np.abs(par.astype(np.float64) - seq) <= 2 * R.bound(y64)).all()


def test_pole_outside_the_unit_circle_takes_the_sequential_instance():
    K = _K()
    b, a = [1.0], [1.0, -1.2]
    assert K.lfilter_instance(b, a) == K.LFILTER_SEQ
    x = _rows(33)
    got = K.lfilter(_dev(x), b, a).cpu().numpy()
    assert R.excess(got, R.reference(x, b, a)) <= 1.0


# ---- shapes and dtypes --------------------------------------------------------------------------------------------------------------------
def test_more_rows_than_a_grid_axis():
    K = _K()
    b, a = R.FILTERS['lowpass100']
    x = R.signal_rows(5, 70000, 33)
    y64 = R.reference(x, b, a)
    for inst in (K.LFILTER_PARALLEL, K.LFILTER_SEQ):
        got = K.lfilter(_dev(x), b, a, instance=inst).cpu().numpy()
        assert R.excess(got, y64) <= 1.0
    got = K.lfilter(_dev(x), b, a, reverse=True).cpu().numpy()
    assert R.excess(got, R.reference(x, b, a, True)) <= 1.0


def test_shapes_views_and_empty_inputs():
    K, snd = _K(), _snd()
    b, a = R.FILTERS['lowpass100']
    x = _dev(_rows(2049))
    y = K.lfilter(x, b, a)
    assert torch.equal(K.lfilter(x.reshape(3, 1, 2049), b, a), y.reshape(3, 1, 2049))
    assert torch.equal(K.lfilter(x[1], b, a), y[1]) and K.lfilter(x[1], b, a).shape == (2049,)
    xt = x.t().contiguous().t()                                         # (3, 2049) with strides (1, 3)
    assert not xt.is_contiguous() and torch.equal(K.lfilter(xt, b, a), y)
    wide = _dev(R.signal_rows(6, 40, 50))
    cols = wide.t()                                                     # time along the strided axis
    assert R.excess(K.lfilter(cols, b, a).cpu().numpy(), R.reference(wide.cpu().numpy().T, b, a)) <= 1.0
    for shape in ((0, 100), (4, 0), (0, 0), (2, 0, 7)):
        e = torch.empty(shape, device=DEV)
        for inst in (K.LFILTER_PARALLEL, K.LFILTER_SEQ):
            out = K.lfilter(e, b, a, instance=inst)
            assert out.shape == shape and out.is_cuda
    assert snd.lowpass(x, 100).shape == x.shape and torch.equal(snd.lowpass(x, 100), y)
    assert torch.equal(snd.biquad(x, b, a), y)
    assert R.excess(snd.highpass(x, 80).cpu().numpy(), R.reference(_rows(2049), *R.FILTERS['highpass80'])) <= 1.0


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_half_precisions_are_cast_in_and_out(dtype):
    K = _K()
    b, a = R.FILTERS['lowpass100']
    x = _dev(_rows(8193)).to(dtype)
    for reverse in (False, True):
        y = K.lfilter(x, b, a, reverse=reverse)
        assert y.dtype == dtype and y.is_cuda
        assert torch.equal(y, K.lfilter(x.float(), b, a, reverse=reverse).to(dtype))      # the float32 result rounded once
    xg = x.clone().requires_grad_(True)
    K.lfilter(xg, b, a).sum().backward()
    assert xg.grad.dtype == dtype and torch.isfinite(xg.grad).all()


def test_float64_raises_on_hip_tensors():
    K = _K()
    with pytest.raises(K.PsndError, match='float64'):
        K.lfilter(torch.zeros(2, 64, dtype=torch.float64, device=DEV), [1.0], [1.0, -0.97])
    with pytest.raises(K.PsndError):
        K.lfilter(torch.zeros(2, 64, dtype=torch.int32, device=DEV), [1.0], [1.0, -0.97])


# ---- gradient -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['pole+0.97', 'lowpass20', 'fir'])
def test_input_gradient_is_the_mirrored_filter(name):
    K = _K()
    b, a = R.FILTERS[name]
    g = R.signal_rows(77, 3, BIG)
    want = R.reference(g, b, a, reverse=True)
    runs = []
    for _ in range(2):
        x = _dev(_rows(BIG)).requires_grad_(True)
        y = K.lfilter(x, b, a)
        (gx,) = torch.autograd.grad(y, x, _dev(g))
        runs.append(gx)
    e = R.excess(runs[0].cpu().numpy(), want)
    _report('gradient %s' % name, e)
    assert e <= 1.0
    assert torch.equal(runs[0], runs[1])                                # no atomics, fixed orders: the same bits


def test_gradient_through_the_inverse_pair_is_all_ones():
    snd = _snd()
    x = _dev(_rows(BIG)).requires_grad_(True)
    y = snd.inv_preemphasis(snd.preemphasis(x))
    assert (y - x).abs().max().item() <= 1e-6
    y.sum().backward()
    assert (x.grad - 1.0).abs().max().item() <= 1e-5


def test_second_derivative_composes():
    K = _K()
    b, a = R.FILTERS['lowpass100']
    x = _dev(_rows(8193)).requires_grad_(True)
    g = _dev(R.signal_rows(78, 3, 8193)).requires_grad_(True)
    u = _dev(R.signal_rows(79, 3, 8193))
    (gx,) = torch.autograd.grad(K.lfilter(x, b, a), x, g, create_graph=True)
    (d,) = torch.autograd.grad(gx, g, u)
    assert torch.equal(d, K.lfilter(u, b, a))


# ---- capture and memory -------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_replay_from_a_graph():
    K = _K()
    b, a = R.FILTERS['lowpass20']
    x = _dev(_rows(BIG)).requires_grad_(True)
    g = _dev(R.signal_rows(80, 3, BIG))

    def step():
        y = K.lfilter(x, b, a)
        (gx,) = torch.autograd.grad(y, x, g)
        return y, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                       # one stream, no parallel branches
        y_s, gx_s = step()
    new_x, new_g = _dev(R.signal_rows(81, 3, BIG)), _dev(R.signal_rows(82, 3, BIG))
    with torch.no_grad():
        x.copy_(new_x)
        g.copy_(new_g)
    y_s.zero_()
    gx_s.zero_()
    graph.replay()
    torch.cuda.synchronize()
    y_e, gx_e = step()
    assert y_s.abs().max() > 0 and torch.equal(y_s, y_e) and torch.equal(gx_s, gx_e)
    assert R.excess(y_s.detach().cpu().numpy(), R.reference(new_x.cpu().numpy(), b, a)) <= 1.0


@pytest.mark.parametrize('name', ['lowpass20', 'pole+0.97'])
def test_same_bits_on_poisoned_memory(name):
    """the carry scratch, the output and the gradient come from torch.empty: every entry read must have been written by the path"""
    K = _K()
    b, a = R.FILTERS[name]
    x = _dev(_rows(BIG))
    g = _dev(R.signal_rows(83, 3, BIG))

    def fn():
        xr = x.clone().requires_grad_(True)
        y = K.lfilter(xr, b, a)
        (gx,) = torch.autograd.grad(y, xr, g)
        return [y, gx, K.lfilter(x, b, a, instance=K.LFILTER_SEQ)]

    first = P.assert_same_bits(fn)
    assert R.excess(first[0].numpy(), _ref(name, BIG, False)) <= 1.0


def test_no_library_op_is_reached():
    from test_gpu_no_library_paths import forbid_library_ops
    snd = _snd()
    x = _dev(_rows(8193)).requires_grad_(True)
    with forbid_library_ops():
        y = snd.lowpass(snd.inv_preemphasis(snd.preemphasis(x)), 100) + snd.highpass(x.to(torch.bfloat16), 80).float()
        y.sum().backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0


# ---- non-finite input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['pole+0.97', 'lowpass100'])
def test_a_nan_does_not_travel_backwards_in_time(name):
    K = _K()
    b, a = R.FILTERS[name]
    x = _dev(_rows(8193))
    clean = K.lfilter(x, b, a)
    bad = x.clone()
    bad[:, 5000] = float('nan')
    for inst in (K.LFILTER_PARALLEL, K.LFILTER_SEQ):
        y = K.lfilter(bad, b, a, instance=inst)
        ref = clean if inst == K.LFILTER_PARALLEL else K.lfilter(x, b, a, instance=inst)
        assert torch.equal(y[:, :5000], ref[:, :5000]) and torch.isnan(y[:, 5000]).all()
