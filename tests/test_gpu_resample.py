"""Sample-rate conversion on HIP tensors (psnd_resample.hip): every seam of the tiling in both directions, impulse rows bit for bit,
asymmetric taps, autograd, shapes and dtypes, utils.sound.resample and models.sound.Resample, graph capture, memory the path did not write,
library ops, and a NaN in the input.  Yardstick and bound: tests/resample_ref.py."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as R  # noqa: E402
import poison as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TILE = 1024
# factors of two and three, the usual audio pairs, a second pure decimation (up = 1 shares each tap among a lane's outputs), and two decimations steep enough that a
# tile's span of x is staged in more than one piece (1024 down / up > 3072)
RATIOS = ((2, 1), (1, 2), (3, 2), (2, 3), (160, 147), (147, 320), (320, 441), (1, 3), (1, 4), (3, 22))


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _snd():
    import pytorch_sound.utils.sound as m
    return m


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                         # a copy: the cached rows are read-only


@functools.lru_cache(maxsize=None)
def _taps(up, down):
    h = R.taps(up, down)
    h.setflags(write=False)
    return h, h.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _rows(seed, T, N=3):
    x = R.signal_rows(seed, N, T)
    x.setflags(write=False)
    return x


def _targets(K):
    return sorted({1, 2, max(K - 1, 1), K, K + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5})


def _adjoint_call(g, up, down, T):
    """the adjoint called directly: factors exchanged, taps reversed, the length given"""
    K = _K()
    return K.ResampleFn.apply(g, down, up, K.resample_plan(up, down), True, T, None)


def test_constants_match_the_header():
    K = _K()
    assert K.RESAMPLE_TILE == TILE


# ---- seams --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('up,down', RATIOS)
def test_seams_both_directions(up, down):
    K = _K()
    h64, h32 = _taps(up, down)
    worst = {'forward': 0.0, 'adjoint': 0.0}
    # forward: input lengths whose output lengths sit on the targets - floor(t down / up) gives exactly t where down >= up, the ceiling the
    # next length an interpolation can reach - and the odd T next to each
    lengths = {1, 2, 3}
    for t in _targets(R.max_products(h64.size, up)):
        for T0 in (max(t * down // up, 1), -(-t * down // up)):
            lengths |= {T0, T0 | 1}
    reached = set()
    for T in sorted(lengths):
        x = _rows(100 + T, T)
        xd = _dev(x)
        assert T % 2 == 0 or xd[1].data_ptr() % 16 != 0                  # an odd T puts rows 1 and 2 off a 16-byte boundary
        got = K.resample_poly(xd, up, down)
        T_out = R.out_len(T, up, down)
        reached.add(T_out)
        assert got.shape == (3, T_out) and got.dtype == torch.float32 and got.is_cuda
        e = R.excess(got.cpu().numpy(), R.resample(x, up, down, h64), R.bound(x, h32, up, down, T_out))
        worst['forward'] = max(worst['forward'], e)
        assert e <= 1.0, ('forward', up, down, T, e)
    if up <= down:                                                       # a decimation reaches every output length
        assert set(_targets(R.max_products(h64.size, up))) <= reached
    # adjoint: its output has the length of the forward input, so T itself sits on the targets
    for T in sorted({1, 2, 3} | set(_targets(R.max_products(h64.size, down)))):
        T_out = R.out_len(T, up, down)
        g = _rows(200 + T, T_out)
        gd = _dev(g)
        assert T_out % 2 == 0 or gd[1].data_ptr() % 16 != 0
        got = _adjoint_call(gd, up, down, T)
        assert got.shape == (3, T) and got.dtype == torch.float32
        e = R.excess(got.cpu().numpy(), R.adjoint(g, up, down, T, h64), R.bound(g, h32[::-1], down, up, T))
        worst['adjoint'] = max(worst['adjoint'], e)
        assert e <= 1.0, ('adjoint', up, down, T, e)
    for k, v in worst.items():
        print('%d/%d %s: worst |error| / bound = %.3f' % (up, down, k, v))


# ---- impulses: indexing and the flip, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('up,down', RATIOS)
def test_impulse_rows_reproduce_the_taps(up, down):
    K = _K()
    h64, h32 = _taps(up, down)
    Ph = h32.size // 2
    for T in (1, 37, 2 * TILE + 3):
        x = np.zeros((2, T), dtype=np.float32)
        x[0, 0] = 1.0
        x[1, T - 1] = 1.0
        T_out = R.out_len(T, up, down)
        got = K.resample_poly(_dev(x), up, down).cpu().numpy()
        want = np.zeros((2, T_out), dtype=np.float32)
        for m in range(T_out):                                           # one product, one term: y[m] = fp32(h[m down - i up + P])
            for r, i in ((0, 0), (1, T - 1)):
                k = m * down - i * up + Ph
                if 0 <= k < h32.size:
                    want[r, m] += h32[k]
        assert np.array_equal(got, want), (up, down, T)
        # the adjoint of an impulse at output m: gx[i] = fp32(h[m down - i up + P])
        g = np.zeros((2, T_out), dtype=np.float32)
        g[0, 0] = 1.0
        g[1, T_out - 1] = 1.0
        got = _adjoint_call(_dev(g), up, down, T).cpu().numpy()
        want = np.zeros((2, T), dtype=np.float32)
        for i in range(T):
            for r, m in ((0, 0), (1, T_out - 1)):
                k = m * down - i * up + Ph
                if 0 <= k < h32.size:
                    want[r, i] += h32[k]
        assert np.array_equal(got, want), ('adjoint', up, down, T)


@pytest.mark.parametrize('up,down', [(2, 3), (3, 2), (16, 21)])
def test_asymmetric_custom_taps(up, down):
    """taps 1 ... 7: not symmetric, so a missing or a doubled flip shows; at 16 / 21 most phases hold no tap at all"""
    K = _K()
    w = np.arange(1.0, 8.0)
    h = w * up                                                           # as scipy applies an array given for window=
    for T in (1, 23, TILE + 7):
        x = _rows(300 + T, T)
        xd = _dev(x).requires_grad_(True)
        y = K.resample_poly(xd, up, down, taps=w)
        T_out = R.out_len(T, up, down)
        assert R.excess(y.detach().cpu().numpy(), R.resample(x, up, down, h), R.bound(x, h, up, down, T_out)) <= 1.0
        g = _rows(400 + T, T_out)
        (gx,) = torch.autograd.grad(y, xd, _dev(g))
        assert R.excess(gx.cpu().numpy(), R.adjoint(g, up, down, T, h), R.bound(g, h[::-1], down, up, T)) <= 1.0
    x = np.zeros((1, 9), dtype=np.float32)
    x[0, 4] = 1.0
    got = K.resample_poly(_dev(x), up, down, taps=w).cpu().numpy()
    assert np.array_equal(got, R.resample(x, up, down, h).astype(np.float32))     # single products of small integers: exact


# ---- autograd -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('up,down', [(1, 2), (2, 1), (320, 441), (147, 320)])
def test_autograd_is_the_adjoint(up, down):
    K = _K()
    h64, h32 = _taps(up, down)
    T = 2 * TILE + 77
    T_out = R.out_len(T, up, down)
    x, g = _rows(500, T), _rows(501, T_out)
    runs = []
    for _ in range(2):
        xd = _dev(x).requires_grad_(True)
        y = K.resample_poly(xd, up, down)
        y.backward(_dev(g))
        runs.append((y.detach(), xd.grad))
    y, gx = runs[0]
    assert torch.equal(gx, runs[1][1]) and torch.equal(y, runs[1][0])    # no atomics, fixed orders: the same bits
    by, bg = R.bound(x, h32, up, down, T_out), R.bound(g, h32[::-1], down, up, T)
    e = R.excess(gx.cpu().numpy(), R.adjoint(g, up, down, T, h64), bg)
    print('%d/%d gradient: worst |error| / bound = %.3f' % (up, down, e))
    assert e <= 1.0
    # <y, g> = <x, gx>: each side is off by at most sum |g| bound(y) and sum |x| bound(gx) - together at most (K + 3) 2^-23 of the mass
    lhs = (y.cpu().numpy().astype(np.float64) * g).sum()
    rhs = (x.astype(np.float64) * gx.cpu().numpy()).sum()
    slack = (np.abs(g) * by).sum() + (np.abs(x) * bg).sum()
    print('%d/%d <y, g> - <x, gx> = %.3e, allowed %.3e' % (up, down, lhs - rhs, slack))
    assert abs(lhs - rhs) <= slack
    # the gradient of the gradient is a forward call
    xd = _dev(x).requires_grad_(True)
    gd = _dev(g).requires_grad_(True)
    u = _dev(_rows(502, T))
    (gx2,) = torch.autograd.grad(K.resample_poly(xd, up, down), xd, gd, create_graph=True)
    (d,) = torch.autograd.grad(gx2, gd, u)
    assert torch.equal(d, K.resample_poly(u, up, down))


# ---- shapes and dtypes --------------------------------------------------------------------------------------------------------------------
def test_shapes_views_and_empty_inputs():
    K = _K()
    up, down = 320, 441
    h64, h32 = _taps(up, down)
    T = 2049
    T_out = R.out_len(T, up, down)
    x = R.signal_rows(7, 6, T)                                           # all four kinds of row, the constant one included
    xd = _dev(x)
    y = K.resample_poly(xd, up, down)
    assert R.excess(y.cpu().numpy(), R.resample(x, up, down, h64), R.bound(x, h32, up, down, T_out)) <= 1.0
    assert torch.equal(K.resample_poly(xd.reshape(2, 3, T), up, down), y.reshape(2, 3, T_out))
    one = K.resample_poly(xd[1], up, down)
    assert one.shape == (T_out,) and torch.equal(one, y[1])
    wide = _dev(R.signal_rows(8, 6, 2 * T))
    strided = wide[:, ::2]                                               # a strided slice
    assert not strided.is_contiguous() and torch.equal(K.resample_poly(strided, up, down), K.resample_poly(strided.contiguous(), up, down))
    for shape, want in (((0, 100), (0, R.out_len(100, up, down))), ((4, 0), (4, 0)), ((0, 0), (0, 0)), ((2, 0, 7), (2, 0, R.out_len(7, up, down))),
                        ((2, 3, 0), (2, 3, 0))):
        out = K.resample_poly(torch.empty(shape, device=DEV), up, down)
        assert out.shape == want and out.is_cuda
    # T == 0 into a given length: zeros
    z = K.ResampleFn.apply(torch.empty(3, 0, device=DEV), up, down, K.resample_plan(up, down), False, 5, None)
    assert z.shape == (3, 5) and not z.any()
    same = K.resample_poly(xd, 5, 5)
    assert torch.equal(same, xd) and same.data_ptr() != xd.data_ptr()


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16])
def test_half_precisions_are_cast_in_and_out(dtype):
    K = _K()
    x = _dev(_rows(9, 2049)).to(dtype)
    for up, down in ((1, 2), (320, 441)):
        y = K.resample_poly(x, up, down)
        assert y.dtype == dtype and y.is_cuda
        assert torch.equal(y, K.resample_poly(x.float(), up, down).to(dtype))          # the float32 result rounded once
    xg = x.clone().requires_grad_(True)
    K.resample_poly(xg, 3, 2).sum().backward()
    assert xg.grad.dtype == dtype and xg.grad.shape == x.shape and torch.isfinite(xg.grad).all()


def test_what_raises_on_hip_tensors():
    K = _K()
    with pytest.raises(K.PsndError, match='float64'):
        K.resample_poly(torch.zeros(2, 64, dtype=torch.float64, device=DEV), 1, 2)
    with pytest.raises(K.PsndError, match='floating'):
        K.resample_poly(torch.zeros(2, 64, dtype=torch.int32, device=DEV), 1, 2)
    with pytest.raises(K.PsndError):
        K.resample_poly(torch.zeros((), device=DEV), 1, 2)
    with pytest.raises(K.PsndError, match=r'1 / 641.*%d' % K.RESAMPLE_MAX_TAPS):          # 12821 taps: refused before any launch
        K.resample_poly(torch.zeros(2, 64, device=DEV), 1, 641)
    with pytest.raises(K.PsndError, match='device taps'):
        K.resample_poly(torch.zeros(2, 64, device=DEV), 1, 2, device_taps=torch.zeros(41))
    assert K.resample_poly(torch.zeros(2, 700, dtype=torch.float64), 1, 641).shape == (2, 2)    # a CPU tensor has no such limit


# ---- the public functions -----------------------------------------------------------------------------------------------------------------
def test_utils_sound_and_the_module_on_hip_tensors():
    from pytorch_sound.models.sound import Resample
    K, snd = _K(), _snd()
    x = _dev(_rows(10, 2049))
    for rates in ((44100, 22050), (22050, 16000), (16000, 48000)):
        up, down = K.resample_ratio(*rates)
        want = K.resample_poly(x, up, down)
        got = snd.resample(x, *rates)
        assert got.is_cuda and got.dtype == torch.float32 and torch.equal(got, want)
        m = Resample(*rates).to(DEV)
        assert m.taps.is_cuda and m.state_dict() == {}
        assert torch.equal(m(x), want) and torch.equal(m(x.reshape(3, 1, 2049)), want.reshape(3, 1, -1))
        assert m(x.to(torch.bfloat16)).dtype == torch.bfloat16
        xg = x.clone().requires_grad_(True)
        m(xg).sum().backward()
        xr = x.clone().requires_grad_(True)
        want_g = torch.autograd.grad(K.resample_poly(xr, up, down).sum(), xr)[0]
        assert torch.equal(xg.grad, want_g)
    with pytest.raises(K.PsndError, match='device taps'):
        Resample(2, 1)(x)                                                # the module was left on the host


def test_down_and_up_again_returns_a_sine():
    """44100 -> 22050 -> 44100 of a 1 kHz sine.  What the pair of filters does to it is taken from the float64 definition on the same
    input; the float32 path may add its derived bound: that of the second sum on what the first one may have produced, and the first
    one's bound carried through the second filter."""
    snd = _snd()
    T = 4410
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(T) / 44100.0)).astype(np.float32)[None]
    ha, hb = _taps(1, 2), _taps(2, 1)
    mid64 = R.resample(x, 1, 2, ha[0])
    back64 = R.resample(mid64, 2, 1, hb[0])
    b_mid = R.bound(x, ha[1], 1, 2, mid64.shape[-1])
    b_back = R.bound(np.abs(mid64) + b_mid, hb[1], 2, 1, T) + R.resample(b_mid, 2, 1, np.abs(hb[1]).astype(np.float64))
    mid = snd.resample(_dev(x), 44100, 22050)
    back = snd.resample(mid, 22050, 44100)
    assert back.shape == (1, T) and back.is_cuda
    got = back.cpu().numpy().astype(np.float64)
    assert (np.abs(got - back64) <= b_back).all()
    edge = 2 * (ha[0].size // 2)                                         # 2P samples at each end feel the zeros beyond the signal
    inner = slice(edge, T - edge)
    own = np.abs(back64 - x)[0, inner].max()
    err = np.abs(got - x)[0, inner].max()
    print('round trip: filters alone %.3e, on the device %.3e, float32 bound %.3e' % (own, err, b_back[0, inner].max()))
    assert err <= own + b_back[0, inner].max()


# ---- capture and memory -------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_replay_from_a_graph():
    K = _K()
    up, down = 320, 441
    T = 2 * TILE + 77
    T_out = R.out_len(T, up, down)
    x = _dev(_rows(11, T)).requires_grad_(True)
    g = _dev(_rows(12, T_out))

    def step():
        y = K.resample_poly(x, up, down)
        (gx,) = torch.autograd.grad(y, x, g)
        return y, gx

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    taps = K.resample_plan(up, down).on(x.device)                        # made by the warm-up: the capture copies nothing from the host
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                        # one stream, one chain, no parallel branches
        y_s, gx_s = step()
    assert K.resample_plan(up, down).on(x.device) is taps
    new_x, new_g = _dev(_rows(13, T)), _dev(_rows(14, T_out))
    with torch.no_grad():
        x.copy_(new_x)
        g.copy_(new_g)
    y_s.zero_()
    gx_s.zero_()
    graph.replay()
    torch.cuda.synchronize()
    y_e, gx_e = step()
    assert y_s.abs().max() > 0 and torch.equal(y_s, y_e) and torch.equal(gx_s, gx_e)
    h64, h32 = _taps(up, down)
    assert R.excess(y_s.detach().cpu().numpy(), R.resample(_rows(13, T), up, down, h64), R.bound(_rows(13, T), h32, up, down, T_out)) <= 1.0


@pytest.mark.parametrize('up,down', [(1, 2), (320, 441), (3, 22)])
def test_same_bits_on_poisoned_memory(up, down):
    """the output and the gradient come from torch.empty: every entry read must have been written by the path"""
    K = _K()
    T = 2 * TILE + 77
    x = _dev(_rows(15, T))
    g = _dev(_rows(16, R.out_len(T, up, down)))

    def fn():
        xr = x.clone().requires_grad_(True)
        y = K.resample_poly(xr, up, down)
        (gx,) = torch.autograd.grad(y, xr, g)
        return [y, gx]

    first = P.assert_same_bits(fn)
    h64, h32 = _taps(up, down)
    assert R.excess(first[0].numpy(), R.resample(_rows(15, T), up, down, h64), R.bound(_rows(15, T), h32, up, down, first[0].shape[-1])) <= 1.0


@pytest.mark.parametrize('up,down,T', [(1, 2, 2 * TILE + 1), (320, 441, 1411), (2, 1, 3), (3, 22, 1)])
def test_nothing_is_written_beside_the_output(up, down, T):
    """the C entry on an output that lies inside a larger buffer: guard bands in front of it and behind it keep their poison, and a
    poisoned output gives the bits of a fresh one"""
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr
    K = _K()
    N, GUARD = 3, 4096
    T_out = R.out_len(T, up, down)
    x = _dev(_rows(17, T))
    want = K.resample_poly(x, up, down)
    taps = K.resample_plan(up, down).on(x.device)
    for byte in P.PATTERNS:
        word = int.from_bytes(bytes([byte] * 4), 'little', signed=True)
        buf = torch.full((2 * GUARD + N * T_out,), word, dtype=torch.int32, device=DEV)
        y = buf[GUARD:GUARD + N * T_out].view(torch.float32)
        rc = lib().psnd_resample(ptr(x), N, T, ptr(taps), taps.numel(), up, down, 0, ctypes.c_void_p(y.data_ptr()), T_out, stream_ptr(x.device))
        assert rc == 0
        torch.cuda.synchronize()
        assert P.same_bits(y.reshape(N, T_out), want), hex(byte)
        assert bool((buf[:GUARD] == word).all()) and bool((buf[GUARD + N * T_out:] == word).all()), hex(byte)


def test_no_library_op_is_reached():
    from test_gpu_no_library_paths import forbid_library_ops
    snd = _snd()
    x = _dev(_rows(18, 2049)).requires_grad_(True)
    with forbid_library_ops():
        y = snd.resample(x, 44100, 22050)
        z = snd.resample(y, 22050, 16000) + snd.resample(x.to(torch.bfloat16), 44100, 16000).float()
        z.sum().backward()
    assert torch.isfinite(x.grad).all() and x.grad.abs().max() > 0


# ---- non-finite input ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('up,down', [(1, 2), (2, 1), (320, 441), (3, 22)])
@pytest.mark.parametrize('value', [float('nan'), float('inf')])
def test_a_nan_reaches_the_outputs_that_cover_it_and_no_others(up, down, value):
    K = _K()
    h64, _ = _taps(up, down)
    T = TILE + 301
    x = _rows(19, T).copy()
    clean = K.resample_poly(_dev(x), up, down)
    for i in (0, 700, T - 1):
        bad = x.copy()
        bad[:, i] = value
        got = K.resample_poly(_dev(bad), up, down)
        with np.errstate(invalid='ignore'):
            want = ~np.isfinite(R.resample(bad, up, down, h64))          # inf times a tap of either sign, or their sum: inf or NaN
        mask = ~torch.isfinite(got).cpu().numpy()
        assert want.any() and np.array_equal(mask, want), (up, down, i)
        keep = torch.from_numpy(~want).to(DEV)
        assert torch.equal(got[keep], clean[keep])
