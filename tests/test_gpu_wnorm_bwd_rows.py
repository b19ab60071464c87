"""Weight-norm backward of the convs (psnd_conv1d_wnorm_bwd, psnd_conv1d_wnorm_bwd_multi) after the lean path of the 256-thread launches
went from one output channel per workgroup to eight (psnd_conv.hip: conv_finish_rows): the sums keep their grouping - per virtual thread
an FMA chain over its quads, a 64-lane butterfly per virtual wave, the wave sums in order, the slabs in order - so g_v, g_g and g_bias are
compared bit for bit with fixtures recorded from the kernels before the change (tests/golden/wnorm_rows_*.npz, written by
tools/gen_wnorm_bwd_golden.py; the inputs come from the seeds below).

Every output lies in front of a guard region of one channel row filled with a sentinel, and the padded tail of g_bias holds the sentinel
too: nothing outside the result may be written.  Cases b and d are also checked against the float64 formula, to the tolerance of the
weight-norm gradients in tests/test_gpu_conv.py (test_fused_conv_fwd_bwd: 3e-2 relative Frobenius)."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SENTINEL = -12345.0
VALUE_TOL = 3e-2            # tests/test_gpu_conv.py, test_fused_conv_fwd_bwd: relf(weight_v.grad), relf(weight_g.grad)


def conv(Cout, Cin, k, splits, Ca=None, Cb=None, bias=True):
    return dict(Cout=Cout, Cin=Cin, k=k, splits=splits, Ca=Ca or Cin, Cb=Cb or Cout, bias=bias)


# name: (entry point, convs of the launch)
CASES = {
    'a': ('single', [conv(9, 8, 3, 1, bias=False)]),       # a last group with one live channel, n4 = 6, one slab in the 2-slot instance
    'b': ('single', [conv(16, 256, 3, 2)]),                # the flagship row: 3 live virtual waves of 4, two full groups
    'c': ('single', [conv(8, 84, 7, 3)]),                  # n4 = 147; natural-order quads straddle ci; 4 slots, one dead
    'd': ('single', [conv(10, 128, 11, 5)]),               # n4 = 352: two quads per virtual thread; 8 slots; a partial last group
    'e': ('single', [conv(8, 64, 3, 16)]),                 # the 16-slot instance, full
    'f': ('multi', [conv(24, 32, 3, 2), conv(5, 13, 3, 2), conv(12, 20, 3, 4, Ca=32, Cb=32)]),   # both roles in one launch, padded strides
    'g': ('multi', [conv(8, 256, 11, 2), conv(16, 32, 3, 2)]),                                   # n = 2816: the 1024-thread launch
}


def case_inputs(name):
    """per conv (gw_part (S, k, Cb, Ca), gbias_part (S, Cb), v (Cout, Cin, k), g (Cout)) from a fixed seed; a few slab values are -0, 0
    and large, so that the zero terms of the sums and their order show in the bits"""
    out = []
    for i, c in enumerate(CASES[name][1]):
        rs = np.random.RandomState(1000 * (ord(name) - ord('a') + 1) + i)
        gw = rs.randn(c['splits'], c['k'], c['Cb'], c['Ca']).astype(np.float32)
        gw.reshape(-1)[::13] = -0.0
        gw.reshape(-1)[5::29] = 0.0
        gw.reshape(-1)[3::31] *= 4096.0
        gb = rs.randn(c['splits'], c['Cb']).astype(np.float32)
        gb[:, 0] = -0.0
        v = (0.05 * rs.randn(c['Cout'], c['Cin'], c['k'])).astype(np.float32)
        g = (1.0 + 0.3 * rs.rand(c['Cout'])).astype(np.float32)
        out.append((gw, gb, v, g))
    return out


def guarded(numel, guard):
    return torch.full((numel + guard,), SENTINEL, dtype=torch.float32, device=DEV)


def run_case(name, entry=None):
    """launch the case; returns per conv (gv, gg, gbias or None) as numpy arrays and asserts that every guard region is intact"""
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check, WnormDesc
    entry = entry or CASES[name][0]
    convs = CASES[name][1]
    keep, outs, descs = [], [], (WnormDesc * len(convs))()
    for d, c, (gw, gb, v, g) in zip(descs, convs, case_inputs(name)):
        n = c['Cin'] * c['k']
        t = [torch.from_numpy(x).to(DEV) for x in (gw, gb, v, g)]
        o = (guarded(c['Cout'] * n, n), guarded(c['Cout'], n), guarded(c['Cb'], n) if c['bias'] else None)
        keep.append(t)
        outs.append(o)
        d.gw_part, d.gbias_part, d.v, d.g = t[0].data_ptr(), t[1].data_ptr() if c['bias'] else None, t[2].data_ptr(), t[3].data_ptr()
        d.gv, d.gg, d.gbias = o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr() if c['bias'] else None
        d.splits, d.Cout, d.Cin, d.k, d.Cb, d.Ca = c['splits'], c['Cout'], c['Cin'], c['k'], c['Cb'], c['Ca']
    if entry == 'multi':
        check(lib().psnd_conv1d_wnorm_bwd_multi(ctypes.addressof(descs), len(convs), stream_ptr(DEV)), 'psnd_conv1d_wnorm_bwd_multi')
    else:
        for c, t, o in zip(convs, keep, outs):
            check(lib().psnd_conv1d_wnorm_bwd(ptr(t[0]), ptr(t[1]) if c['bias'] else None, c['splits'], ptr(t[2]), ptr(t[3]), c['Cout'], c['Cin'],
                                              c['k'], c['Cb'], c['Ca'], ptr(o[0]), ptr(o[1]), ptr(o[2]), stream_ptr(DEV)), 'psnd_conv1d_wnorm_bwd')
    torch.cuda.synchronize()
    res = []
    for c, o in zip(convs, outs):
        n = c['Cin'] * c['k']
        gv, gg, gb = o[0].cpu().numpy(), o[1].cpu().numpy(), None if o[2] is None else o[2].cpu().numpy()
        assert (gv[c['Cout'] * n:] == SENTINEL).all() and (gg[c['Cout']:] == SENTINEL).all(), (name, 'write behind g_v / g_g')
        assert gb is None or (gb[c['Cout']:] == SENTINEL).all(), (name, 'write behind g_bias')
        for x in (gv[:c['Cout'] * n], gg[:c['Cout']]) + (() if gb is None else (gb[:c['Cout']],)):
            assert not (x == SENTINEL).any() and not np.isnan(x).any(), (name, 'result not written')
        res.append((gv[:c['Cout'] * n].reshape(c['Cout'], c['Cin'], c['k']), gg[:c['Cout']], None if gb is None else gb[:c['Cout']]))
    return res


def golden_path(name):
    return os.path.join(GOLD, 'wnorm_rows_%s.npz' % name)


def same_bits(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)).view(torch.int32), torch.from_numpy(np.ascontiguousarray(b)).view(torch.int32))


@pytest.mark.parametrize('name', sorted(CASES))
def test_bits_of_the_kernels_before_the_row_groups(name):
    """g_v, g_g and g_bias of every case, bit for bit; the single-conv cases through psnd_conv1d_wnorm_bwd and as a launch of one through
    psnd_conv1d_wnorm_bwd_multi (one body, one result)"""
    gold = np.load(golden_path(name))
    for entry in {CASES[name][0], 'multi'}:
        for i, (gv, gg, gb) in enumerate(run_case(name, entry)):
            assert same_bits(gv, gold['gv%d' % i]), (name, entry, i, 'g_v')
            assert same_bits(gg, gold['gg%d' % i]), (name, entry, i, 'g_g')
            assert gb is None or same_bits(gb, gold['gb%d' % i]), (name, entry, i, 'g_bias')


def relf(a, b):
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-12))


@pytest.mark.parametrize('name', ['b', 'd'])
def test_values_against_the_float64_formula(name):
    """g_g = sum(gw * vhat), g_v = (g / ||v||) (gw - vhat g_g), g_bias = sum of the bias slabs, in float64 from the inputs alone"""
    for c, (gw, gb, v, g), (gv, gg, gbias) in zip(CASES[name][1], case_inputs(name), run_case(name)):
        w = gw.astype(np.float64).sum(0)[:, :c['Cout'], :c['Cin']].transpose(1, 2, 0)          # (Cout, Cin, k)
        v64 = v.astype(np.float64)
        norm = np.sqrt((v64 * v64).sum((1, 2), keepdims=True))
        vhat = v64 / norm
        gg_ref = (w * vhat).sum((1, 2))
        gv_ref = g.astype(np.float64).reshape(-1, 1, 1) / norm * (w - vhat * gg_ref.reshape(-1, 1, 1))
        assert relf(gg, gg_ref) < VALUE_TOL and relf(gv, gv_ref) < VALUE_TOL, (name, relf(gg, gg_ref), relf(gv, gv_ref))
        assert relf(gbias, gb.astype(np.float64).sum(0)[:c['Cout']]) < VALUE_TOL
