"""The plain weight-gradient body (conv_wgrad_body, no gradient combine, 64-channel tiles, three taps per workgroup) can stage its row chunks by
LDS-DMA into a ring of chunk slots, several chunks ahead, in a source-swizzled 128-byte-pitch image: the batched launch does, the single
launch and the paired backward launches do under the lab library's PSND_WGRAD_STAGE=dma; every other form keeps the register-staged loop.  What can go wrong with a ring: a chunk read before it landed or after its slot was refilled, a range shorter than the ring, a partial
last chunk, rows / channel pieces out of range that do not arrive as zeros, a swizzle term that differs between the fill and a tap's read, a
ring row nobody filled.  So every case fills the slabs with NaN, launches once, and wants every element finite, BIT-equal to the
register-staged loop (lab library, PSND_WGRAD_STAGE=regs: same products in the same order) and, summed over the slabs, within
test_wgrad_multi_mixed_shapes_vs_float64's 2e-5 of the largest entry of the float64 product of the same bf16 operands.  Lp = 48 throughout:
N = 2 with 2 row ranges gives ranges of 64 and 32 rows (2 and 1 chunks, fewer than the ring holds), N = 7 in one range 336 rows = 10.5 chunks,
N = 8 in one range 12 whole chunks."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

LP = 48
BODY = (256, 256, 3)
# name -> (N, [(Ca, Cb, k, off0, dstep, splits or None = what the helper returns)], with bias slabs)
MULTI = {
    'ranges_shorter_than_the_ring_dilations_1_3_5': (2, [BODY + (-1, 1, None), BODY + (-3, 3, None), BODY + (-5, 5, None)], True),
    'ten_and_a_half_chunks': (7, [BODY + (-1, 1, 1), BODY + (-5, 5, 1)], True),
    'twelve_whole_chunks': (8, [BODY + (-3, 3, 1)], True),
    'seven_taps_three_tap_groups': (2, [(256, 256, 7, -9, 3, None)], True),
    'one_and_two_taps': (7, [(256, 256, 1, 0, 1, 1), (256, 256, 2, -1, 1, 1), (256, 256, 2, 0, 5, 1)], True),
    'mixed_shapes_Ca520_Cb64_Cb40': (2, [BODY + (-1, 1, None), (520, 256, 3, -1, 1, None), (256, 64, 3, -3, 3, None), (256, 40, 3, -5, 5, None)], True),
    'channel_edges_over_a_partial_chunk': (7, [(520, 40, 3, -3, 3, 1)], True),
    'no_bias_slabs': (7, [BODY + (-1, 1, 2), (520, 64, 3, -5, 5, 2)], False),
}


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _ref64(g, x, k, off0, dstep):
    """float64 product of the bf16 operands: (k, Cb, Ca), and the bias sums (Cb)"""
    R = g.shape[0] * g.shape[1]
    G, X = g.double().reshape(R, -1), x.double().reshape(R, -1)
    ref = torch.zeros(k, G.shape[1], X.shape[1], dtype=torch.float64, device=g.device)
    for j in range(k):
        o = off0 + j * dstep
        lo, hi = max(0, -o), min(R, R - o)
        ref[j] = G[lo:hi].t() @ X[lo + o:hi + o]
    return ref, G.sum(0)


def _operands(specs, N, dev, seed=11):
    torch.manual_seed(seed)
    return [(torch.randn(N, LP, Cb, device=dev).to(torch.bfloat16), torch.randn(N, LP, Ca, device=dev).to(torch.bfloat16))
            for Ca, Cb, k, off0, dstep, S in specs]


def _multi(specs, ops, N, bias, S0, dev):
    """one psnd_conv1d_cl_wgrad_multi launch on NaN-filled slabs -> [(gw, gb)]"""
    from pytorch_sound_amd import _lib
    from pytorch_sound_amd._lib import lib, stream_ptr, check
    arr = (_lib.WgradDesc * len(specs))()
    out = []
    for d, (Ca, Cb, k, off0, dstep, S), (g, x) in zip(arr, specs, ops):
        S = S or S0
        gw = torch.full((S, k, Cb, Ca), float('nan'), device=dev)
        gb = torch.full((S, Cb), float('nan'), device=dev) if bias else None
        d.g, d.xa, d.gw_part, d.gbias_part = g.data_ptr(), x.data_ptr(), gw.data_ptr(), _ptr(gb)
        d.off0, d.dstep, d.Ca, d.Cb, d.k, d.splits = off0, dstep, Ca, Cb, k, S
        out.append((gw, gb))
    check(lib().psnd_conv1d_cl_wgrad_multi(ctypes.addressof(arr), len(specs), N, LP, stream_ptr(dev)), 'psnd_conv1d_cl_wgrad_multi')
    torch.cuda.synchronize(dev)
    return out


def _check(name, i, got, regs, g, x, k, off0, dstep):
    """got / regs: (gw, gb) of the default (LDS-DMA where it applies) and of the register-staged loop"""
    (gw, gb), (gw1, gb1) = got, regs
    assert bool(torch.isfinite(gw).all()), (name, i, 'slab elements left unwritten or not finite: %d' % int((~torch.isfinite(gw)).sum()))
    assert bool(torch.isfinite(gw1).all()), (name, i)
    assert torch.equal(gw.view(torch.int32), gw1.view(torch.int32)), (name, i, 'slabs differ from the register-staged loop: %d elements'
                                                                      % int((gw.view(torch.int32) != gw1.view(torch.int32)).sum()))
    ref, bref = _ref64(g, x, k, off0, dstep)
    err, top = float((gw.double().sum(0) - ref).abs().max()), float(ref.abs().max())
    print('%s conv %d: %d slabs, |err| %.3g of %.3g' % (name, i, gw.shape[0], err, top))
    assert err <= 2e-5 * top, (name, i, err, top)
    if gb is not None:
        assert bool(torch.isfinite(gb).all()), (name, i, 'bias slab elements left unwritten')
        assert torch.equal(gb.view(torch.int32), gb1.view(torch.int32)), (name, i, 'bias slabs differ from the register-staged loop')
        assert float((gb.double().sum(0) - bref).abs().max()) <= 2e-5 * float(bref.abs().max()), (name, i)


@pytest.mark.parametrize('name', list(MULTI))
def test_multi_launch_matches_register_staging_and_float64(name, monkeypatch, lab_lib):
    from pytorch_sound_amd._lib import lib
    N, specs, bias = MULTI[name]
    dev = torch.device('cuda:0')
    S0 = lib().psnd_conv1d_cl_wgrad_multi_splits(N, LP, 256, 256, 3, len(specs))
    assert S0 >= 1
    ops = _operands(specs, N, dev)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'dma')
    got = _multi(specs, ops, N, bias, S0, dev)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'regs')
    regs = _multi(specs, ops, N, bias, S0, dev)
    for i, ((Ca, Cb, k, off0, dstep, S), (g, x)) in enumerate(zip(specs, ops)):
        _check(name, i, got[i], regs[i], g, x, k, off0, dstep)


def _single(g, x, N, Ca, Cb, k, off0, dstep, dev, g2=None, gm=None, slope=1.0):
    from pytorch_sound_amd._lib import lib, stream_ptr, check
    S = lib().psnd_conv1d_cl_wgrad_splits(N, LP, Ca, Cb, k)
    assert S >= 1
    gw = torch.full((S, k, Cb, Ca), float('nan'), device=dev)
    gb = torch.full((S, Cb), float('nan'), device=dev)
    check(lib().psnd_conv1d_cl_wgrad(_ptr(g), _ptr(g2), _ptr(gm), slope, _ptr(x), N, LP, Ca, Cb, k, off0, dstep, _ptr(gw), _ptr(gb), None,
                                     stream_ptr(dev)), 'psnd_conv1d_cl_wgrad')
    torch.cuda.synchronize(dev)
    return gw, gb


@pytest.mark.parametrize('N,Ca,Cb,k,off0,dstep', [(2, 256, 256, 3, -1, 1), (7, 520, 256, 3, -1, 1), (7, 256, 40, 7, -9, 3), (8, 256, 64, 2, 0, 5)])
def test_single_launch_matches_register_staging_and_float64(N, Ca, Cb, k, off0, dstep, monkeypatch, lab_lib):
    dev = torch.device('cuda:0')
    (g, x), = _operands([(Ca, Cb, k, off0, dstep, None)], N, dev, seed=12)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'dma')
    got = _single(g, x, N, Ca, Cb, k, off0, dstep, dev)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'regs')
    regs = _single(g, x, N, Ca, Cb, k, off0, dstep, dev)
    _check('wgrad', 0, got, regs, g, x, k, off0, dstep)


def test_combined_gradient_keeps_the_register_path(monkeypatch, lab_lib):
    """g = G1 + G2 * leaky'(GM) is formed in registers on the way into LDS: no LDS-DMA form.  Slope 0.5: the product is exact, so the
    float32 sum rounds once whether the compiler contracts it or not, and the bf16 operand of the reference is the kernel's."""
    dev = torch.device('cuda:0')
    N, Ca, Cb, k, off0, dstep = 7, 256, 256, 3, -3, 3
    torch.manual_seed(13)
    g1, g2, gm = (torch.randn(N, LP, Cb, device=dev).to(torch.bfloat16) for _ in range(3))
    x = torch.randn(N, LP, Ca, device=dev).to(torch.bfloat16)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'dma')
    got = _single(g1, x, N, Ca, Cb, k, off0, dstep, dev, g2, gm, 0.5)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'regs')
    regs = _single(g1, x, N, Ca, Cb, k, off0, dstep, dev, g2, gm, 0.5)
    g = (g1.float() + g2.float() * torch.where(gm.float() > 0, 1.0, 0.5)).to(torch.bfloat16)
    _check('combined', 0, got, regs, g, x, k, off0, dstep)


def _pair_bwd_role(g, x, N, off0, dstep, dev):
    """psnd_conv1d_cl_pair_bwd carrying nothing but a weight-gradient role (the flush of a residual chain's last conv)"""
    from pytorch_sound_amd._lib import lib, stream_ptr, check
    C, k, L, HP = 256, 3, 40, 4
    S = lib().psnd_conv1d_cl_pair_bwd_splits(N, LP, C, k)
    assert S >= 1
    gw = torch.full((S, k, C, C), float('nan'), device=dev)
    gb = torch.full((S, C), float('nan'), device=dev)
    check(lib().psnd_conv1d_cl_pair_bwd(None, None, None, 1.0, None, None, None, 1.0, None, N, LP, L, HP, C, k, 0, 1, 0, 1, None, None, None, None,
                                        _ptr(g), _ptr(x), off0, dstep, _ptr(gw), _ptr(gb), stream_ptr(dev)), 'psnd_conv1d_cl_pair_bwd')
    torch.cuda.synchronize(dev)
    return gw, gb


@pytest.mark.parametrize('N,dil', [(2, 1), (7, 5)])
def test_pair_backward_launch_weight_gradient_role(N, dil, monkeypatch, lab_lib):
    dev = torch.device('cuda:0')
    (g, x), = _operands([BODY + (-dil, dil, None)], N, dev, seed=14)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'dma')
    got = _pair_bwd_role(g, x, N, -dil, dil, dev)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'regs')
    regs = _pair_bwd_role(g, x, N, -dil, dil, dev)
    _check('pair_bwd', 0, got, regs, g, x, 3, -dil, dil)


def _conv_bwd(g, x, wb, N, C, k, dil, dev):
    """psnd_conv1d_cl_bwd: input gradient and weight-gradient role in one launch (conv_bwd_pair_kernel) -> (gw, gb), gx"""
    from pytorch_sound_amd._lib import lib, stream_ptr, check
    L, HP = 32, 8
    S = lib().psnd_conv1d_cl_wgrad_splits(N, LP, C, C, k)
    assert S >= 1
    gw = torch.full((S, k, C, C), float('nan'), device=dev)
    gb = torch.full((S, C), float('nan'), device=dev)
    gx = torch.zeros(N, LP, C, device=dev, dtype=torch.bfloat16)
    check(lib().psnd_conv1d_cl_bwd(_ptr(g), None, None, 1.0, _ptr(wb), _ptr(x), N, LP, L, HP, C, C, k, dil, dil, _ptr(gx), None, None, 1.0, None,
                                   _ptr(gw), _ptr(gb), stream_ptr(dev)), 'psnd_conv1d_cl_bwd')
    torch.cuda.synchronize(dev)
    return (gw, gb), gx


@pytest.mark.parametrize('N,dil', [(2, 3), (7, 1)])
def test_conv_backward_launch_weight_gradient_role(N, dil, monkeypatch, lab_lib):
    dev = torch.device('cuda:0')
    C, k = 256, 3
    (g, x), = _operands([BODY + (-dil, dil, None)], N, dev, seed=15)
    wb = (torch.randn(k, C, C, device=dev) * 0.05).to(torch.bfloat16)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'dma')
    got, gx = _conv_bwd(g, x, wb, N, C, k, dil, dev)
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'regs')
    regs, gx1 = _conv_bwd(g, x, wb, N, C, k, dil, dev)
    assert torch.equal(gx.view(torch.int16), gx1.view(torch.int16)), 'the input-gradient role changed with the weight-gradient staging'
    _check('conv_bwd', 0, got, regs, g, x, k, -dil, dil)


def test_no_result_depends_on_what_lds_held(monkeypatch, lab_lib):
    """A launch over NaN operands leaves NaN in the ring slots (and in the epilogue tile) of every CU; the launches behind it - ranges shorter
    than the ring, a partial last chunk, channel pieces past Cb / Ca - must give the bits they give on their own: rows and pieces out of range
    arrive as zeros from the transfer itself, and ring rows that no chunk fills are never read."""
    from pytorch_sound_amd._lib import lib
    dev = torch.device('cuda:0')
    monkeypatch.setenv('PSND_WGRAD_STAGE', 'dma')
    cases = [MULTI[n] for n in ('ranges_shorter_than_the_ring_dilations_1_3_5', 'channel_edges_over_a_partial_chunk', 'mixed_shapes_Ca520_Cb64_Cb40')]
    runs = []
    for N, specs, bias in cases:
        S0 = lib().psnd_conv1d_cl_wgrad_multi_splits(N, LP, 256, 256, 3, len(specs))
        ops = _operands(specs, N, dev)
        runs.append((N, specs, bias, S0, ops, _multi(specs, ops, N, bias, S0, dev)))
    # 8 body convs over 8 clips: 768 workgroups, three per CU
    pN, pspecs = 8, [BODY + (-1, 1, None)] * 8
    pS0 = lib().psnd_conv1d_cl_wgrad_multi_splits(pN, LP, 256, 256, 3, len(pspecs))
    nan = torch.full((pN, LP, 256), float('nan'), device=dev).to(torch.bfloat16)
    for N, specs, bias, S0, ops, clean in runs:
        _multi(pspecs, [(nan, nan)] * len(pspecs), pN, True, pS0, dev)
        again = _multi(specs, ops, N, bias, S0, dev)
        for i, ((gw, gb), (gw0, gb0)) in enumerate(zip(again, clean)):
            assert bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gb).all()), (specs[i], 'what LDS held reached the slabs')
            assert torch.equal(gw.view(torch.int32), gw0.view(torch.int32)) and torch.equal(gb.view(torch.int32), gb0.view(torch.int32)), specs[i]
