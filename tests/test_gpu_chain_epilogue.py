"""The chain kernel's epilogues (psnd_conv_chain.hip) keep the accumulators channel-contiguous: a lane holds ONE tile row and 16 channels,
packs four channels into one 8-byte LDS store, masks the word with its row's in-clip mask, reads its bias as float4s from an LDS table
and (masked form) its leaky' bits from one word per row block.  What that layout can get wrong - the per-lane row mask, the channel
index of the bias, the bit of the mask word, the address of the 8-byte store - shows as a difference against one pair launch per pair
(the same arithmetic in the transposed accumulator layout) and against the plain-torch emulation of the rounding points."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def relf(a, b):
    a, b = a.detach().float(), b.detach().float()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _chain_stats():
    from pytorch_sound_amd import _lib
    out = (ctypes.c_longlong * 2)()
    _lib.lib().psnd_conv_chain_stats(ctypes.addressof(out))
    return out[0], out[1]


def _model(blocks, seed, distinct_bias=False):
    from pytorch_sound_amd.models import build_model
    from pytorch_sound_amd.models import separator  # noqa: F401
    torch.manual_seed(seed)
    model = build_model('conv_separator_voicebank', {'channels': 256, 'num_blocks': blocks}).to(torch.device('cuda:0'))
    if distinct_bias:
        # every conv: a ramp over its channels, another scale and sign per conv - no two channels of a conv share a value, none is zero
        with torch.no_grad():
            biases = [p for n, p in model.named_parameters() if n.endswith('bias')]
            assert len(biases) == 6 * blocks + 2
            for i, b in enumerate(biases):
                n = b.numel()
                b.copy_((torch.arange(n, device=b.device, dtype=torch.float32) + 1) / n * (0.5 + 0.1 * i) * (-1.0) ** i)
                assert int((b != 0).sum()) == n and b.unique().numel() == n
    return model


def _run(model, mag, tgt, fn=None):
    model.zero_grad()
    m = mag.clone().requires_grad_(True)
    s0 = _chain_stats()
    out = (fn or model)(m)
    (out - tgt).abs().mean().backward()
    s1 = _chain_stats()
    return (s1[0] - s0[0], s1[1] - s0[1]), out.detach().clone(), m.grad.clone(), {k: p.grad.clone() for k, p in model.named_parameters()}


def _chain_vs_pairs(N, T, blocks, chain, mr, monkeypatch, distinct_bias=False):
    dev = torch.device('cuda:0')
    model = _model(blocks, 100 * N + T, distinct_bias)
    mag = torch.rand(N, 513, T, device=dev) * 4
    tgt = torch.rand(N, 513, T, device=dev)
    if mr == 1:
        monkeypatch.setenv('PSND_CHAIN_MR', '1')
    monkeypatch.setenv('PSND_CL_CHAIN', str(chain))
    st1, o1, gm1, g1 = _run(model, mag, tgt)
    monkeypatch.setenv('PSND_CL_CHAIN', '0')
    st0, o0, gm0, g0 = _run(model, mag, tgt)
    assert st0 == (0, 0), st0
    assert st1[0] >= 2 and st1[1] >= 4, st1          # forward and masked chain launches, at least two pairs each
    assert torch.isfinite(o0).all() and float(gm0.abs().max()) > 0
    assert torch.equal(o1, o0)
    assert torch.equal(gm1, gm0)
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k


# (1, 20): a clip shorter than a tile - halo rows inside every tile; (3, 43): one row more than the 42 owned; 64 frames; two blocks of
# 4-pair chains over several workgroups; the 32-row tile instances
@pytest.mark.parametrize('N,T,blocks,chain,mr', [(1, 20, 1, 3, 2), (3, 43, 1, 3, 2), (2, 64, 1, 2, 2), (5, 97, 2, 4, 2),
                                                 (3, 43, 1, 3, 1), (2, 50, 1, 2, 1)])
def test_chain_is_bit_identical_to_pair_launches(N, T, blocks, chain, mr, monkeypatch, lab_lib):
    """forward and backward with PSND_CL_CHAIN=<chain> against PSND_CL_CHAIN=0 (one pair launch per pair): output, input gradient and
    every parameter gradient are bit-equal, and the chain kernel really ran"""
    _chain_vs_pairs(N, T, blocks, chain, mr, monkeypatch)


def test_distinct_bias_per_channel(monkeypatch, lab_lib):
    """every conv's bias a ramp of distinct non-zero values: a slip in the channel a lane reads its bias for cannot hide behind the
    small random biases of a fresh model"""
    _chain_vs_pairs(3, 43, 1, 3, 2, monkeypatch, distinct_bias=True)


def test_chain_vs_bf16_emulation(monkeypatch, lab_lib):
    """the independent reference (tests/bf16_emul.py: the kernels' rounding points in plain torch), 3 clips x 43 frames, one block, with
    the tolerances of test_separator_bench_shape_vs_bf16_emulation for the same quantities"""
    import bf16_emul as E
    dev = torch.device('cuda:0')
    model = _model(1, 343, distinct_bias=True)
    mag = torch.rand(3, 513, 43, device=dev) * 4
    tgt = torch.rand(3, 513, 43, device=dev) * 4
    monkeypatch.setenv('PSND_CL_CHAIN', '3')
    st, o, gx, g = _run(model, mag, tgt)
    assert st == (2, 6), st
    _, eo, egx, eg = _run(model, mag, tgt, lambda m: E.separator(model, m))
    names = sorted(g)
    errs = {'out': relf(o, eo), 'gx': relf(gx, egx),
            'all': relf(torch.cat([g[n].flatten() for n in names]), torch.cat([eg[n].flatten() for n in names]))}
    each = sorted(((relf(g[n], eg[n]), n) for n in names if eg[n].norm() > 0), reverse=True)
    print(errs, each[:3])
    assert errs['out'] <= 1e-3 and errs['gx'] <= 3e-2 and errs['all'] <= 3e-3, errs
    assert each[0][0] <= 1e-2, each[:3]


def test_rows_outside_the_clip_are_written_as_zeros(lab_lib):
    """a forward chain launch at one clip of 20 frames (one workgroup, halo rows inside its tile), called directly: every row outside
    [HP, HP + L) of every tensor the launch writes (mid, raw, activated of each pair) is exactly zero - the per-lane row mask - and the
    rows inside are not"""
    from pytorch_sound_amd import _lib
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    dev = torch.device('cuda:0')
    N, L, HP, C, k, npairs = 1, 20, 5, 256, 3, 3
    Lp = (L + 2 * HP + 7) // 8 * 8
    torch.manual_seed(20)
    x = torch.zeros(N, Lp, C, device=dev, dtype=torch.bfloat16)
    x[:, HP:HP + L] = torch.randn(N, L, C, device=dev).to(torch.bfloat16)
    ws = [(torch.randn(3, C, C, device=dev) / 28).to(torch.bfloat16) for _ in range(2 * npairs)]
    bs = [(torch.arange(C, device=dev, dtype=torch.float32) + 1) / C * (1 + i) for i in range(2 * npairs)]
    outs = [[torch.ones_like(x) for _ in range(3)] for _ in range(npairs)]
    dils = [1, 3, 5]
    arr = (_lib.ChainPair * npairs)()
    for i, d in enumerate(arr):
        d.W1, d.bias1, d.act1_slope, d.mid_out = ws[2 * i].data_ptr(), bs[2 * i].data_ptr(), 0.1, outs[i][0].data_ptr()
        d.W2, d.bias2, d.off1, d.dstep1, d.off2, d.dstep2 = ws[2 * i + 1].data_ptr(), bs[2 * i + 1].data_ptr(), -dils[i], dils[i], -1, 1
        d.act2_slope, d.out_raw, d.out_act = 0.1, outs[i][1].data_ptr(), outs[i][2].data_ptr()
    s0 = _chain_stats()
    with torch.cuda.device(dev):
        check(lib().psnd_conv1d_cl_chain(ptr(x), ptr(x), ctypes.addressof(arr), npairs, N, Lp, L, HP, C, k, stream_ptr(dev)), 'chain')
    torch.cuda.synchronize()
    s1 = _chain_stats()
    assert (s1[0] - s0[0], s1[1] - s0[1]) == (1, npairs)
    for i in range(npairs):
        for name, t in zip(('mid', 'raw', 'act'), outs[i]):
            t = t.float()
            assert float(t[:, :HP].abs().max()) == 0.0 and float(t[:, HP + L:].abs().max()) == 0.0, (i, name)
            assert torch.isfinite(t).all() and int((t[:, HP:HP + L] != 0).sum()) > L * C // 2, (i, name)
