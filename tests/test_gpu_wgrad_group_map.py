"""psnd_conv1d_cl_wgrad_multi numbers its workgroups so that the tiles of one (conv, row range) share an L2 (conv_wgrad_multi_kernel: label =
block % 8, the label's groups one after the other, grid padded to 8 x the heaviest label).  A wrong numbering leaves slab tiles unwritten,
writes a tile twice over different row ranges, or hands a block the wrong conv - so every case fills the slabs with NaN, launches once, and
wants every element finite, BIT-equal to the same conv computed alone (an n = 1 launch with the same row ranges: same body, same sums in
the same order) and, summed over the slabs, within test_wgrad_multi_mixed_shapes_vs_float64's 2e-5 of the largest entry of the float64
product of the same bf16 operands.  Shapes: the smallest that reach each branch of the map (N = 2, Lp = 48: 96 rows, 2 row ranges)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

BODY = (256, 256, 3)
# name -> (N, [(Ca, Cb, k, off0, dstep, splits or None = what the helper returns)], with bias slabs)
CASES = {
    'uniform3_groups_not_a_multiple_of_8': (2, [BODY + (-1, 1, None), BODY + (-3, 3, None), BODY + (-5, 5, None)], True),
    'uniform8_one_group_short_of_two_per_label': (2, [BODY + (-d, d, None) for d in (1, 1, 3, 1, 5, 1, 1, 3)], True),
    'uniform9_past_the_label_count': (2, [BODY + (-d, d, None) for d in (1, 1, 3, 1, 5, 1, 1, 3, 1)], True),
    'mixed_shapes_padded_grid': (2, [BODY + (-1, 1, None), (520, 256, 3, -1, 1, None), (256, 64, 3, -1, 1, None)], True),
    'seven_taps_three_tap_groups': (2, [(256, 256, 7, -9, 3, None)], True),
    'splits_differ_per_descriptor': (8, [BODY + (-1, 1, 1), BODY + (-3, 3, 2), BODY + (-5, 5, 3), BODY + (-1, 1, 2)], True),
    'no_bias_slabs': (2, [BODY + (-1, 1, None), BODY + (-3, 3, None), BODY + (-5, 5, None)], False),
}
LP = 48


def _launch(arr, n, N, dev):
    from pytorch_sound_amd._lib import lib, stream_ptr, check
    check(lib().psnd_conv1d_cl_wgrad_multi(ctypes.addressof(arr), n, N, LP, stream_ptr(dev)), 'psnd_conv1d_cl_wgrad_multi')


def _fill(d, g, x, gw, gb, spec, S):
    Ca, Cb, k, off0, dstep, _ = spec
    d.g, d.xa, d.gw_part, d.gbias_part = g.data_ptr(), x.data_ptr(), gw.data_ptr(), gb.data_ptr() if gb is not None else None
    d.off0, d.dstep, d.Ca, d.Cb, d.k, d.splits = off0, dstep, Ca, Cb, k, S


@pytest.mark.parametrize('name', list(CASES))
def test_group_map_writes_every_slab_tile_once(name):
    from pytorch_sound_amd import _lib
    from pytorch_sound_amd._lib import lib
    N, specs, bias = CASES[name]
    dev = torch.device('cuda:0')
    torch.manual_seed(11)
    R = N * LP
    S0 = lib().psnd_conv1d_cl_wgrad_multi_splits(N, LP, 256, 256, 3, len(specs))
    assert S0 >= 1
    arr = (_lib.WgradDesc * len(specs))()
    keep = []
    for d, spec in zip(arr, specs):
        Ca, Cb, k, off0, dstep, S = spec
        S = S or S0
        g = torch.randn(N, LP, Cb, device=dev).to(torch.bfloat16)
        x = torch.randn(N, LP, Ca, device=dev).to(torch.bfloat16)
        gw = torch.full((S, k, Cb, Ca), float('nan'), device=dev)
        gb = torch.full((S, Cb), float('nan'), device=dev) if bias else None
        _fill(d, g, x, gw, gb, spec, S)
        keep.append((g, x, gw, gb, S))
    _launch(arr, len(specs), N, dev)
    for i, (spec, (g, x, gw, gb, S)) in enumerate(zip(specs, keep)):
        Ca, Cb, k, off0, dstep, _ = spec
        assert bool(torch.isfinite(gw).all()), (name, i, 'slab elements left unwritten: %d' % int((~torch.isfinite(gw)).sum()))
        # the same conv alone: same row ranges, same body
        one = (_lib.WgradDesc * 1)()
        gw1 = torch.full_like(gw, float('nan'))
        gb1 = torch.full_like(gb, float('nan')) if bias else None
        _fill(one[0], g, x, gw1, gb1, spec, S)
        _launch(one, 1, N, dev)
        assert bool(torch.isfinite(gw1).all())
        assert torch.equal(gw.view(torch.int32), gw1.view(torch.int32)), (name, i, 'slabs differ from the conv computed alone')
        G = g.double().reshape(R, Cb)
        X = x.double().reshape(R, Ca)
        ref = torch.zeros(k, Cb, Ca, dtype=torch.float64, device=dev)
        for j in range(k):
            o = off0 + j * dstep
            lo, hi = max(0, -o), min(R, R - o)
            ref[j] = G[lo:hi].t() @ X[lo + o:hi + o]
        err, top = float((gw.double().sum(0) - ref).abs().max()), float(ref.abs().max())
        print('%s conv %d: %d slabs, |err| %.3g of %.3g' % (name, i, S, err, top))
        assert err <= 2e-5 * top, (name, i, err, top)
        if bias:
            assert bool(torch.isfinite(gb).all()), (name, i, 'bias slab elements left unwritten')
            assert torch.equal(gb.view(torch.int32), gb1.view(torch.int32)), (name, i)
            assert float((gb.double().sum(0) - G.sum(0)).abs().max()) <= 2e-5 * float(G.sum(0).abs().max())
