"""The attention kernels (psnd_mha_fwd / _bwd: csrc/psnd_attn.hip) and psnd_softmax_keys_* where the other tests never take them:
padding masks that are no suffix (a masked first key tile, a masked tile between live ones, single holes, every other frame, a whole
128-query tile of padding inside a clip, a clip that is padding only), sequence lengths on and next to the 32-key / 128-query tile edges
(T = 1 included), T beyond the 512-tile key-bit table in LDS, and softmax columns with |logit| up to ~190.

Reference: the torch formulation of modules.py:61-79 in float64 (`_attention_float64` of test_gpu_modules; `_attention_ref` below is the
same function in any dtype and in query chunks - the CPU test at the end of this file pins that the two agree and pins the reference's
semantics the GPU tests assert EXACTLY: padded key rows / padded query columns of att are 0, out at padded queries is 0, the gradients
of K, V at padded keys and of Q at padded queries are 0, a clip of padding only gives zeros and no NaN, live columns sum to 1).

Tolerance rule (the one of test_config4_block_vs_float64): the allowance is the LARGER of
  * the bound the existing test of that kernel instance uses - fp32: 1e-5 relative Frobenius (out), 1e-4 (gradient), 2e-6 absolute
    (probabilities); bf16 operands: 2e-3 (two-pass) / 4e-3 (one-pass) of max against float64 on the ROUNDED operands (out), 2e-6 + 1e-4
    max p (probabilities), 2e-2 relative Frobenius (gradient) - test_attention_fp32_single_pass_forward, test_attention_bf16_operands,
    test_attention_bf16_single_pass_forward; kvq STORED as bf16: out is also stored as bf16, half an ulp = 2^-9 of the element on top;
  * TWICE the error of the same formulation in plain torch ops in fp32 (for the bf16 modes: with the same straight-through bf16 rounding
    of K, Q, V and the probabilities) against float64 on the same input - computed here, never taken from the kernels.
The module-level tests run their float64 and fp32 references on the CPU: a float64 HIP tensor handed to the modules is cast to fp32 and
takes the kernels (models/modules.py `_to_kernel_dtype`), it would be no reference."""
import functools

import pytest
import torch

from test_gpu_modules import _attention_float64

gpu = pytest.mark.gpu
DEV = torch.device('cuda:0')
NEG_INF = float('-inf')


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------------------
def edge_masks(T):
    """(6, T) bool, True = padding: (a) a prefix of 40 frames - the first 32-key tile masked, the second partly; (b) holes - frames 32..63
    (a whole key tile between live ones), 100..130 and the single frames 0, 31, T - 1; (c) every other frame; (d) frames 128..255, a whole
    128-query tile, live frames on both sides (T < 257: up to T - 2); (e) every frame; (f) none"""
    m = torch.zeros(6, T, dtype=torch.bool)
    m[0, :40] = True
    m[1, 32:64] = True
    m[1, 100:131] = True
    m[1, [0, 31, T - 1]] = True
    m[2, ::2] = True
    m[3, 128:min(256, T - 1)] = True
    m[4, :] = True
    return m


def _attention_ref(kvq, mask, H, gout, gatt, round_operands, dtype, chunk=None):
    """`_attention_float64` in `dtype` (float32: the yardstick), optionally over `chunk` query columns at a time (the softmax runs over
    the keys: query columns are independent; the K / V gradients add up over the chunks' backward passes) -> out, att (None when
    chunked), gkvq"""
    N, C3, T = kvq.shape
    C = C3 // 3
    d = C // H
    x = kvq.detach().to(dtype).requires_grad_(True)

    class _R(torch.autograd.Function):          # straight-through rounding, as in _attention_float64
        @staticmethod
        def forward(ctx, t):
            return t.float().bfloat16().to(t.dtype)

        @staticmethod
        def backward(ctx, g):
            return g

    r = _R.apply if round_operands else (lambda t: t)
    m = None if mask is None else mask.bool().repeat(H, 1)
    outs, att = [], None
    step = chunk or T
    for q0 in range(0, T, step):
        q1 = min(T, q0 + step)
        k, v, q = (t.view(N, H, d, T).transpose(0, 1).reshape(H * N, d, T) for t in x.chunk(3, 1))
        s = torch.einsum('bdk,bdq->bkq', r(k), r(q[:, :, q0:q1])) / (d ** 0.5)
        if m is not None:
            s = s.masked_fill(m[:, :, None], NEG_INF)
        a = torch.softmax(s, 1)
        if m is not None:
            a = a.masked_fill(m[:, None, q0:q1], 0.0)
        o = torch.einsum('bdk,bkq->bdq', r(v), r(a)).view(H, N, d, q1 - q0).transpose(0, 1).reshape(N, C, q1 - q0)
        loss = (o * gout[:, :, q0:q1].to(dtype)).sum()
        if gatt is not None:
            loss = loss + (a * gatt[:, :, q0:q1].to(dtype)).sum()
        loss.backward()
        outs.append(o.detach())
        if chunk is None:
            att = a.detach()
    return torch.cat(outs, 2), att, x.grad


def _run_kernels(kvq, m8, H, want_att, mode, gout, gatt):
    """K.AttentionKVQ forward + backward -> out, att (None without), gkvq.  mode: 'fp32', 'bf16' (bf16 operands) or 'stored' (kvq a bf16
    tensor: out and the gradient come back as bf16 tensors)"""
    from pytorch_sound_amd import kernels as K
    x = (kvq.to(torch.bfloat16) if mode == 'stored' else kvq).clone().requires_grad_(True)
    out, att = K.AttentionKVQ.apply(x, m8, H, want_att, mode != 'fp32')
    assert out.dtype == x.dtype and (att.numel() > 0) == want_att
    loss = (out.float() * gout).sum()
    if gatt is not None:
        loss = loss + (att * gatt).sum()
    loss.backward()
    torch.cuda.synchronize()
    assert x.grad.dtype == x.dtype
    return out.detach().float(), (att.detach() if want_att else None), x.grad.float()


def _rel(a, b):
    """relative Frobenius error; a reference that is all zeros asks for all zeros"""
    nb = float(b.double().norm())
    e = float((a.double() - b.double()).norm())
    return e / nb if nb > 0 else (0.0 if e == 0 else float('inf'))


def _amax(a, b):
    return float((a.double() - b.double()).abs().max())


def _omax(a, b):
    """largest error as a fraction of the largest reference value"""
    mb = float(b.double().abs().max())
    e = _amax(a, b)
    return e / mb if mb > 0 else (0.0 if e == 0 else float('inf'))


def _refs(kvq, mask, H, gout, gatt, rounded, chunk=None):
    """float64 reference and its fp32 yardstick (both: out, att, gkvq)"""
    if chunk is None:
        r64 = _attention_float64(kvq, mask, H, gout, gatt, rounded)
    else:
        r64 = _attention_ref(kvq, mask, H, gout, gatt, rounded, torch.float64, chunk)
    return r64, _attention_ref(kvq, mask, H, gout, gatt, rounded, torch.float32, chunk)


def _compare(tag, got, mode, want_att, exact, rounded, grad_vs_rounded=False):
    """the tolerance rule of the module docstring.  got: (out, att, gkvq) of the kernels; exact / rounded: `_refs` without / with operand
    rounding (rounded: the bf16 modes only).  Prints every figure next to its yardstick before it asserts; returns them."""
    out, att, g = got
    fig = {}
    if mode == 'fp32':
        (o64, a64, g64), (o32, a32, g32) = exact
        fig['out'] = (_rel(out, o64), _rel(o32, o64), 1e-5)
        fig['grad'] = (_rel(g, g64), _rel(g32, g64), 1e-4)
        if want_att:
            fig['att'] = (_amax(att, a64), _amax(a32, a64), 2e-6)
    else:
        (o64, a64, g64), (o32, a32, g32) = rounded
        fig['out'] = (_omax(out, o64), _omax(o32, o64), (2e-3 if want_att else 4e-3) + (2.0 ** -9 if mode == 'stored' else 0.0))
        if want_att:
            fig['att'] = (_amax(att, a64), _amax(a32, a64), 2e-6 + 1e-4 * float(a64.max()))
        if not grad_vs_rounded:
            (_, _, g64), (_, _, g32) = exact[0], rounded[1]          # against the exact gradient; the yardstick rounds its operands
        fig['grad'] = (_rel(g, g64), _rel(g32, g64), 2e-2)
    print('%s: ' % tag + '  '.join('%s %.1e (torch fp32 %.1e, base %.1e)' % ((k,) + v) for k, v in fig.items()))
    for k, (err, yard, base) in fig.items():
        assert err <= max(base, 2.0 * yard), (tag, k, err, yard, base)
    return fig


def _assert_structure(mask, H, out, att, g):
    """what the reference gives EXACTLY (the CPU test below): nothing non-finite, padded key rows and padded query columns of att are 0,
    out at padded queries is 0, no gradient at a padded frame (K, V: padded key; Q: padded query); live query columns sum to 1"""
    N, T = mask.shape
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
    pad = mask.bool()
    assert float((out * pad[:, None, :]).abs().max()) == 0
    assert float((g * pad[:, None, :]).abs().max()) == 0
    if att is not None:
        assert bool(torch.isfinite(att).all())
        a = att.view(H, N, T, T)
        assert float((a * pad[None, :, :, None]).abs().max()) == 0
        assert float((a * pad[None, :, None, :]).abs().max()) == 0
        colsum = a.double().sum(2)                                    # (H, N, T_query)
        live = (~pad)[None].expand(H, N, T)
        # 1e-5: test_softmax_keys_large_with_mask's bound for the same sum (fp32 probabilities, T <= 1292 terms of relative error 2^-23 each)
        assert float((colsum[live] - 1).abs().max()) <= 1e-5 if bool(live.any()) else True
        assert float(colsum[~live].abs().max()) == 0 if bool((~live).any()) else True


CONFIGS = [('fp32', True, True), ('fp32', True, False), ('fp32', False, False), ('bf16', True, True), ('bf16', True, False),
           ('bf16', False, False), ('stored', False, False)]       # (mode, want_att, gradient into att); the ABI refuses the others
CONFIG_IDS = ['%s-%s%s' % (m, 'att' if a else 'noatt', '-gatt' if g else '') for m, a, g in CONFIGS]


def _inputs(seed, N, H, d, T, mode, with_gatt, sigma=1.0):
    dev = DEV
    gen = torch.Generator(device='cpu').manual_seed(seed)
    C = H * d
    kvq = torch.randn(N, 3 * C, T, generator=gen)
    kvq[:, :C] *= sigma                          # keys and queries scaled: logits grow with sigma^2; values stay at unit variance
    kvq[:, 2 * C:] *= sigma
    gout = torch.randn(N, C, T, generator=gen)
    gatt = 0.3 * torch.randn(H * N, T, T, generator=gen) if with_gatt else None
    if mode == 'stored':                         # the values a bf16 tensor can hold: kernels and references start from the same numbers
        kvq, gout = kvq.bfloat16().float(), gout.bfloat16().float()
    return kvq.to(dev), gout.to(dev), (None if gatt is None else gatt.to(dev))


@functools.lru_cache(maxsize=4)
def _case(seed, N, H, d, T, stored, with_gatt, sigma=1.0, tie=False):
    """inputs on the six clips of `edge_masks`, shared (and left unchanged) by the tests that run several kernel instances on them"""
    kvq, gout, gatt = _inputs(seed, N, H, d, T, 'stored' if stored else 'fp32', with_gatt, sigma)
    if tie:
        kvq = _with_tie(kvq, H, d)
    return kvq, gout, gatt, edge_masks(T).to(kvq.device)


@functools.lru_cache(maxsize=8)
def _case_refs(rounded, *key):
    kvq, gout, gatt, mask = _case(*key)
    return _refs(kvq, mask, key[2], gout, gatt, rounded)


def _with_tie(kvq, H, d):
    """keys 50 and 90 of every head are the same vector and query 70 points along it: column 70 has an exact tie at its maximum"""
    C = H * d
    kvq = kvq.clone()
    kvq[:, :C, 50] = kvq[:, :C, 90]
    kvq[:, 2 * C:, 70] = kvq[:, :C, 90]
    return kvq


# ---------------------------------------------------------------------------------------------------------------------
# 1. mask shapes
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('mode,want_att,with_gatt', CONFIGS, ids=CONFIG_IDS)
@pytest.mark.parametrize('d', [16, 48, 64, 128])
def test_mask_shapes(d, mode, want_att, with_gatt):
    """K.AttentionKVQ on ONE batch of the six clips of `edge_masks` at T = 300 (three 128-query tiles, the last ragged), H = 2: 12 (head,
    clip) pairs - the XCD numbering of attn_tile wraps once and has four padding workgroups per tile -, head dimensions 16 / 48 / 64 /
    128 (the HDP = 32 / 64 / 128 instances, d < HDP and d = HDP), two-pass and one-pass forward, with and without a gradient into att, fp32 /
    bf16 operands / kvq stored as bf16.  out, att and the kvq gradient against float64 on the same mask (module docstring), the exact
    zeros of `_assert_structure`, and every clip but the empty one BIT FOR BIT what it gives alone as a batch of one (a clip's workgroups
    read no other clip).
    MI355X, worst over the four head dimensions, error (torch fp32 yardstick): fp32 out 4.7e-7 (5.1e-7), gradient 4.9e-7 (5.2e-7), att
    2.7e-7 (2.9e-7); bf16 two-pass out 3.1e-4 of max (6.3e-4), att 7.8e-8, gradient 4.4e-3 (3.7e-3: the yardstick's operand rounding
    against the exact gradient); bf16 one-pass out 2.7e-3; stored out 4.4e-3 of 6.0e-3, gradient 2.4e-3; every solo run bit-equal."""
    N, H, T = 6, 2, 300
    key = (d, N, H, d, T, mode == 'stored', with_gatt)
    kvq, gout, gatt, mask = _case(*key)
    m8 = mask.to(torch.uint8)
    got = _run_kernels(kvq, m8, H, want_att, mode, gout, gatt)
    exact = _case_refs(False, *key)
    rounded = _case_refs(True, *key) if mode != 'fp32' else None
    _compare('d=%d %s att=%s gatt=%s' % (d, mode, want_att, with_gatt), got, mode, want_att, exact, rounded)
    out, att, g = got
    _assert_structure(mask, H, out, att, g)
    assert float(out[4].abs().max()) == 0 and float(g[4].abs().max()) == 0          # (e): the clip of padding only
    for c in (0, 1, 2, 3, 5):
        ga = None if gatt is None else gatt.view(H, N, T, T)[:, c].contiguous()
        o1, a1, g1 = _run_kernels(kvq[c:c + 1], m8[c:c + 1], H, want_att, mode, gout[c:c + 1], ga)
        assert torch.equal(out[c], o1[0]) and torch.equal(g[c], g1[0]), c
        if want_att:
            assert torch.equal(att.view(H, N, T, T)[:, c], a1.view(H, T, T)), c


def _module_refs(mha, x0, mask, gy, gatt):
    """MultiHeadAttention forward + backward in float64 and in fp32, torch formulation on the CPU -> (y, att, gx, parameter gradients) each"""
    import copy
    res = []
    for dt in (torch.float64, torch.float32):
        m = copy.deepcopy(mha).cpu().to(dt)
        m.zero_grad()
        x = x0.detach().cpu().to(dt).requires_grad_(True)
        y, att = m(x, mask.cpu())
        ((y * gy.cpu().to(dt)).sum() + (att * gatt.cpu().to(dt)).sum()).backward()
        res.append((y.detach(), att.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()}))
    return res


def _module_check(tag, mha, x0, mask, gy, gatt):
    """the module on HIP tensors against `_module_refs`; bounds of test_config4_block_vs_float64: 3e-5 of max (output), 1e-5 absolute
    (probabilities), 2e-4 of max (gradients) or twice the fp32 yardstick"""
    (yr, ar, gxr, gpr), (y32, a32, gx32, gp32) = _module_refs(mha, x0, mask, gy, gatt)
    mha.zero_grad()
    x = x0.clone().requires_grad_(True)
    y, att = mha(x, mask)
    ((y * gy).sum() + (att * gatt).sum()).backward()
    torch.cuda.synchronize()
    gp = {k: p.grad.cpu() for k, p in mha.named_parameters()}
    y, att, gx = y.detach().cpu(), att.detach().cpu(), x.grad.cpu()
    assert all(bool(torch.isfinite(t).all()) for t in [y, att, gx] + list(gp.values()))
    worst = max(gp, key=lambda k: _omax(gp[k], gpr[k]))
    fig = {'y': (_omax(y, yr), _omax(y32, yr), 3e-5), 'att': (_amax(att, ar), _amax(a32, ar), 1e-5), 'gx': (_omax(gx, gxr), _omax(gx32, gxr), 2e-4),
           'worst param grad': (_omax(gp[worst], gpr[worst]), _omax(gp32[worst], gpr[worst]), 2e-4)}
    print('%s: ' % tag + '  '.join('%s %.1e (torch fp32 %.1e, base %.1e)' % ((k,) + v) for k, v in fig.items()))
    for k, (err, yard, base) in fig.items():
        assert err <= max(base, 2.0 * yard), (tag, k, err, yard, base)
    for k in gp:
        assert _omax(gp[k], gpr[k]) <= max(2e-4, 2.0 * _omax(gp32[k], gpr[k])), (tag, k)
    return y, att, gx, gp


@gpu
def test_mask_shapes_through_the_module():
    """the same six clips as a BOOL mask through MultiHeadAttention.forward (the module hands the kernels a byte view of it) against the
    module in float64 on the CPU; the same mask as uint8 gives the same bits; att keeps its exact zeros.
    MI355X: y 7.3e-8 of max (torch fp32 on the CPU 1.0e-7), att 1.4e-8 (1.7e-8), input gradient 1.2e-7 (1.0e-7), worst parameter gradient
    3.5e-7 (3.6e-7)."""
    from pytorch_sound_amd.models.modules import MultiHeadAttention
    dev = DEV
    torch.manual_seed(3)
    N, C, H, T = 6, 64, 2, 300
    mha = MultiHeadAttention(C, H, 0.0).to(dev)
    x0, gy = torch.randn(N, C, T, device=dev), torch.randn(N, C, T, device=dev)
    gatt = 0.3 * torch.randn(H * N, T, T, device=dev)
    mask = edge_masks(T).to(dev)
    y, att, gx, _ = _module_check('module T=300', mha, x0, mask, gy, gatt)
    pad = mask.cpu()
    a = att.view(H, N, T, T)
    assert float((a * pad[None, :, :, None]).abs().max()) == 0 and float((a * pad[None, :, None, :]).abs().max()) == 0
    x = x0.clone().requires_grad_(True)
    y8, att8 = mha(x, mask.to(torch.uint8))
    ((y8 * gy).sum() + (att8 * gatt).sum()).backward()
    assert torch.equal(y8.detach().cpu(), y) and torch.equal(att8.detach().cpu(), att) and torch.equal(x.grad.cpu(), gx)


# ---------------------------------------------------------------------------------------------------------------------
# 2. tile-edge lengths
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('mode', ['fp32', 'bf16'])
@pytest.mark.parametrize('d', [64, 16])
@pytest.mark.parametrize('T', [1, 2, 31, 32, 33, 64, 127, 128, 129])
def test_tile_edge_lengths(T, d, mode):
    """T on and next to the edges of the 32-key tile and the 128-query tile, and T = 1 / 2 (N = 3, H = 2): without a mask, and with frame 0
    and the last frame padded in the first clip, the last frame in the second, none in the third (T = 1: without a mask, and one clip that
    is padding only; T = 2 with the mask: the first clip is padding only).  Two-pass forward with a gradient into att, and the one-pass
    forward; out, att and the gradient against float64.
    MI355X, worst over all lengths: fp32 out 3.4e-7 (torch fp32 3.7e-7), gradient 3.5e-7 (3.8e-7), att 2.8e-7 (2.8e-7); bf16 out 3.2e-3
    of max on the one-pass form (bound 4e-3; yardstick 1.0e-3), att 1.1e-7, gradient 4.3e-3 (3.6e-3)."""
    N, H = 3, 2
    dev = DEV
    masks = [None]
    m = torch.zeros(N, T, dtype=torch.bool, device=dev)
    if T == 1:
        m[0] = True
    else:
        m[0, 0] = m[0, T - 1] = m[1, T - 1] = True
    masks.append(m)
    for want_att in (True, False):
        kvq, gout, gatt = _inputs(1000 * T + d, N, H, d, T, mode, want_att)
        for mask in masks:
            m8 = None if mask is None else mask.to(torch.uint8)
            got = _run_kernels(kvq, m8, H, want_att, mode, gout, gatt)
            exact = _refs(kvq, mask, H, gout, gatt, False)
            rounded = _refs(kvq, mask, H, gout, gatt, True) if mode != 'fp32' else None
            _compare('T=%d d=%d %s att=%s mask=%s' % (T, d, mode, want_att, mask is not None), got, mode, want_att, exact, rounded)
            _assert_structure(mask if mask is not None else torch.zeros(N, T, dtype=torch.bool, device=dev), H, *got)


# ---------------------------------------------------------------------------------------------------------------------
# 3. beyond the key-bit table
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('mode', ['fp32', 'bf16', 'stored'])
def test_beyond_the_key_bit_table(mode):
    """T = 16384 + 40: key tiles 512 and 513 lie past the table of KBITS_MAX = 512 words in LDS, their words come from key_bits inside
    the loops (forward, query gradient; N = H = 1, d = 16, no att tensor).  The mask pads a prefix, frames below 16384 - the end of the
    last tile the table holds among them - and frames 16390..16400, so the words of tiles 511 and 512 differ and the fallback sees
    masked keys.  float64 reference on the GPU over 1024 query columns at a time.
    MI355X: fp32 out 2.3e-6 (torch fp32 2.2e-6), gradient 2.4e-6 (2.0e-6); bf16 out 2.1e-3 of max (2.5e-4), gradient 4.5e-3 (3.9e-3);
    stored out 2.3e-3, gradient 2.4e-3 (9.0e-4); 1-2 s a case, the chunked references included."""
    N, H, d, T = 1, 1, 16, 16384 + 40
    kvq, gout, _ = _inputs(7, N, H, d, T, mode, False)
    mask = torch.zeros(N, T, dtype=torch.bool, device=kvq.device)
    mask[0, :40] = True
    mask[0, 5000:5100] = True
    mask[0, 16380:16384] = True
    mask[0, 16390:16401] = True
    got = _run_kernels(kvq, mask.to(torch.uint8), H, False, mode, gout, None)
    exact = _refs(kvq, mask, H, gout, None, False, chunk=1024)
    rounded = _refs(kvq, mask, H, gout, None, True, chunk=1024) if mode != 'fp32' else None
    _compare('T=%d %s' % (T, mode), got, mode, False, exact, rounded)
    _assert_structure(mask, H, *got)


# ---------------------------------------------------------------------------------------------------------------------
# 4. sharp softmax
# ---------------------------------------------------------------------------------------------------------------------
SHARP = [(m, a, g, s, False) for m, a, g in CONFIGS if g or not a for s in ((1.0, 2.5, 4.0, 6.0) if m == 'fp32' else (1.0, 2.5))]
SHARP += [('fp32', True, True, 4.0, True), ('fp32', False, False, 4.0, True), ('bf16', True, True, 2.5, True), ('bf16', False, False, 2.5, True),
          ('stored', False, False, 2.5, True)]


@gpu
@pytest.mark.parametrize('mode,want_att,with_gatt,sigma,tie', SHARP,
                         ids=['%s-%s-sigma%g%s' % (m, 'att-gatt' if a else 'noatt', s, '-tie' if t else '') for m, a, g, s, t in SHARP])
def test_sharp_softmax(mode, want_att, with_gatt, sigma, tie):
    """K and Q scaled by sigma, V at unit variance (d = 32, T = 161, H = 2, the six clips of `edge_masks`): the largest |logit| is about
    5, 31, 80 and 188 at sigma = 1, 2.5, 4 and 6 - columns with one probability next to 1 and the rest down to exp(-370): the maximum
    subtraction, the rescaling of the one-pass accumulator, the fused exponent offset of the bf16 backward.  fp32 instances: all four;
    bf16 instances: sigma = 1 and 2.5.  `tie`: two identical keys share a column's maximum.  The bf16 gradient at sigma > 1 is held
    against the float64 gradient on the ROUNDED operands: rounding K and Q moves a logit of 30 by ~0.06 - another function, no error.
    MI355X, error (torch fp32 yardstick) at sigma = 1 / 2.5 / 4 / 6 - fp32 two-pass: out 2.9e-7 (3.3e-7) / 6.8e-7 (5.8e-7) / 1.3e-6
    (7.9e-7) / 2.5e-6 (1.2e-6), gradient 3.1e-7 (3.4e-7) / 1.2e-6 (9.1e-7) / 3.8e-6 (1.9e-6) / 1.3e-5 (4.3e-6), att 1.7e-7 (2.0e-7) /
    1.8e-6 (1.5e-6) / 4.8e-6 (3.9e-6) / 8.8e-6 (8.5e-6) - the probabilities leave the fixed 2e-6 at sigma = 4, inside twice the yardstick;
    fp32 one-pass: out 2.9e-7 / 5.5e-7 / 7.9e-7 / 1.2e-6, gradient 3.0e-7 / 9.4e-7 / 2.1e-6 / 4.6e-6 (the yardstick's own figures).
    bf16 at sigma = 1 / 2.5 - two-pass out 1.5e-4 / 4.7e-7 of max, att 6.0e-8 / 1.1e-6, gradient 3.9e-3 / 4.9e-3; one-pass out 2.5e-3 /
    1.5e-3, gradient 3.9e-3 / 4.1e-3; stored out 4.4e-3 / 3.0e-3 of 6.0e-3, gradient 2.4e-3 / 3.9e-3: all inside the existing bounds
    (2e-3 / 4e-3 of max, 2e-2), none needed the yardstick.  The tie: the two probabilities are the same bits, 0.5 each."""
    N, H, d, T = 6, 2, 32, 161
    key = (int(10 * sigma) + 7 * tie, N, H, d, T, mode == 'stored', with_gatt, sigma, tie)
    kvq, gout, gatt, mask = _case(*key)
    got = _run_kernels(kvq, mask.to(torch.uint8), H, want_att, mode, gout, gatt)
    exact = _case_refs(False, *key)
    rounded = _case_refs(True, *key) if mode != 'fp32' else None
    _compare('sigma=%g tie=%s %s att=%s' % (sigma, tie, mode, want_att), got, mode, want_att, exact, rounded, grad_vs_rounded=sigma > 1)
    _assert_structure(mask, H, *got)
    if tie and want_att:
        a = got[1].view(H, N, T, T)[:, 5, :, 70]                         # clip (f), the query that points along the doubled key
        assert torch.equal(a[:, 50], a[:, 90]) and float(a[:, 50].min()) > 0.4


@gpu
@pytest.mark.parametrize('sigma', [1.0, 2.5, 4.0, 6.0])
def test_sharp_softmax_through_the_module(sigma):
    """MultiHeadAttention(64, 2) in fp32 on an input scaled by sigma (the projection's logits grow with sigma^2), holes in the mask,
    against the module in float64 on the CPU.
    MI355X at sigma = 1 / 2.5 / 4 / 6, error (torch fp32 on the CPU): y 9.2e-8 (1.2e-7) / 7.5e-7 (5.8e-7) / 1.9e-6 (1.9e-6) / 4.5e-6
    (4.4e-6) of max, att 1.5e-7 (1.6e-7) / 2.1e-6 (1.8e-6) / 4.7e-6 (5.0e-6) / 1.3e-5 (1.3e-5), input gradient 1.5e-7 / 1.8e-6 / 5.7e-6 /
    1.3e-5 (1.4e-7 / 1.4e-6 / 3.6e-6 / 1.3e-5), worst parameter gradient 4.7e-7 / 2.2e-6 / 5.3e-6 / 1.9e-5 (4.9e-7 / 1.3e-6 / 3.1e-6 /
    8.3e-6): the probabilities at sigma = 6 pass by the yardstick (1.3e-5 against the fixed 1e-5)."""
    from pytorch_sound_amd.models.modules import MultiHeadAttention
    dev = DEV
    torch.manual_seed(int(10 * sigma))
    N, C, H, T = 6, 64, 2, 161
    mha = MultiHeadAttention(C, H, 0.0).to(dev)
    with torch.no_grad():
        mha.linear_kvq.weight.mul_(3.0 ** 0.5)   # (Conv1d's default weights have variance 1 / (3 C): K and Q of variance sigma^2, as in the kernel tests)
    x0, gy = sigma * torch.randn(N, C, T, device=dev), torch.randn(N, C, T, device=dev)
    gatt = 0.3 * torch.randn(H * N, T, T, device=dev)
    _module_check('module sigma=%g' % sigma, mha, x0, edge_masks(T).to(dev), gy, gatt)


# ---------------------------------------------------------------------------------------------------------------------
# 5. SoftmaxKeys
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('T', [161, 164])
def test_softmax_keys_masks_and_sharp_columns(T):
    """psnd_softmax_keys_fwd / _bwd on the six clips of `edge_masks` with |score * scale| up to ~200 (T = 161: the scalar kernels; 164: the
    16-byte ones, T % 4 == 0), against float64: 2e-6 (the bound of test_softmax_keys_large_with_mask) or twice the error of torch's fp32
    softmax on the same input; exact zeros at padded keys / queries, the empty clip all zero, live columns sum to 1.
    MI355X (largest |score * scale| 201 / 193): att 1.6e-7 / 1.5e-7 (torch fp32 2.0e-7 / 1.4e-7), gradient 3.6e-8 / 4.0e-8 of the largest
    (3.2e-8 / 3.8e-8): inside the fixed 2e-6."""
    from pytorch_sound_amd import kernels as K
    dev = DEV
    torch.manual_seed(T)
    B = 6
    s = torch.randn(B, T, T, device=dev) * 360
    scale = 1.0 / 8.0
    mask = edge_masks(T).to(dev)
    ga = torch.randn(B, T, T, device=dev)

    def ref(dt):
        x = s.detach().to(dt).clone().requires_grad_(True)
        a = torch.softmax((x * scale).masked_fill(mask.unsqueeze(2), NEG_INF), 1).masked_fill(mask.unsqueeze(1), 0.0)
        (a * ga.to(dt)).sum().backward()
        return a.detach(), x.grad

    (a64, g64), (a32, g32) = ref(torch.float64), ref(torch.float32)
    sx = s.detach().clone().requires_grad_(True)
    att = K.SoftmaxKeys.apply(sx, mask.to(torch.uint8), scale)
    (att * ga).sum().backward()
    torch.cuda.synchronize()
    att, gs = att.detach(), sx.grad
    gmax = max(1.0, float(g64.abs().max()))
    fig = {'att': (_amax(att, a64), _amax(a32, a64), 2e-6), 'grad': (_amax(gs, g64) / gmax, _amax(g32, g64) / gmax, 2e-6)}
    print('T=%d largest |score * scale| %.0f: ' % (T, float(s.abs().max()) * scale) +
          '  '.join('%s %.1e (torch fp32 %.1e, base %.1e)' % ((k,) + v) for k, v in fig.items()))
    for k, (err, yard, base) in fig.items():
        assert err <= max(base, 2.0 * yard), (k, err, yard, base)
    assert bool(torch.isfinite(att).all()) and bool(torch.isfinite(gs).all())
    assert float((att * mask[:, :, None]).abs().max()) == 0 and float((att * mask[:, None, :]).abs().max()) == 0
    assert float((gs * mask[:, :, None]).abs().max()) == 0 and float((gs * mask[:, None, :]).abs().max()) == 0
    assert float(att[4].abs().max()) == 0 and float(gs[4].abs().max()) == 0
    live = ~mask
    assert float((att.double().sum(1)[live] - 1).abs().max()) <= 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own semantics, on the CPU (no kernel involved)
# ---------------------------------------------------------------------------------------------------------------------
def test_reference_semantics_on_the_cpu():
    """what the GPU tests above take from the float64 torch formulation, in torch ops alone: a clip of padding only gives out == 0 and
    zero gradients for K, V and Q without a NaN (masked_fill's backward clears the softmax's NaN column), padded key rows / query columns
    of att and the matching outputs and gradients are exact zeros, live columns sum to 1; `_attention_ref` is `_attention_float64` (bit
    for bit unchunked, to rounding when the queries come in chunks) and MultiHeadAttention.scale_dot_att; the SoftmaxKeys formulation
    has the same zeros."""
    from pytorch_sound_amd.models.modules import MultiHeadAttention
    torch.manual_seed(0)
    N, H, d, T = 6, 2, 8, 161
    C = H * d
    mask = edge_masks(T)
    assert bool(mask[4].all()) and not bool(mask[5].any()) and bool(mask[0, :40].all()) and not bool(mask[0, 40:].any())
    assert bool(mask[3, 128:160].all()) and not bool(mask[3, 160]) and bool(edge_masks(300)[3, 128:256].all()) and not bool(edge_masks(300)[3, 256:].any())
    for sigma in (1.0, 6.0):
        kvq = torch.randn(N, 3 * C, T)              # (fp32, as in the GPU tests: _attention_float64 makes its own float64 leaf of it)
        kvq[:, :C] *= sigma
        kvq[:, 2 * C:] *= sigma
        gout, gatt = torch.randn(N, C, T), torch.randn(H * N, T, T)
        for ga in (None, gatt):
            for rounded in (False, True):
                out, att, g = _attention_float64(kvq, mask, H, gout, ga, rounded)
                assert all(bool(torch.isfinite(t).all()) for t in (out, att, g))
                assert float(out[4].abs().max()) == 0 and float(g[4].abs().max()) == 0
                assert float((out * mask[:, None, :]).abs().max()) == 0 and float((g * mask[:, None, :]).abs().max()) == 0
                a = att.view(H, N, T, T)
                assert float((a * mask[None, :, :, None]).abs().max()) == 0 and float((a * mask[None, :, None, :]).abs().max()) == 0
                cs = a.sum(2)
                live = (~mask)[None].expand(H, N, T)
                assert float((cs[live] - 1).abs().max()) <= 1e-12 and float(cs[~live].abs().max()) == 0
                o2, a2, g2 = _attention_ref(kvq, mask, H, gout, ga, rounded, torch.float64)
                assert torch.equal(o2, out) and torch.equal(a2, att) and torch.equal(g2, g)
                o3, _, g3 = _attention_ref(kvq, mask, H, gout, ga, rounded, torch.float64, chunk=64)
                assert _omax(o3, out) <= 1e-12 and _omax(g3, g) <= 1e-12
        k, v, q = (t.view(N, H, d, T).transpose(0, 1).reshape(H * N, d, T) for t in kvq.double().chunk(3, 1))
        xs, atts = MultiHeadAttention.scale_dot_att(k, v, q, mask.repeat(H, 1))
        out, att, _ = _attention_float64(kvq, mask, H, gout, None, False)
        assert _amax(atts, att) <= 1e-12 and _omax(xs.view(H, N, d, T).transpose(0, 1).reshape(N, C, T), out) <= 1e-12
    s = (torch.randn(N, T, T, dtype=torch.float64) * 360).requires_grad_(True)
    a = torch.softmax((s / 8.0).masked_fill(mask.unsqueeze(2), NEG_INF), 1).masked_fill(mask.unsqueeze(1), 0.0)
    (a * torch.randn(N, T, T, dtype=torch.float64)).sum().backward()
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(s.grad).all())
    a = a.detach()
    assert float(a[4].abs().max()) == 0 and float(s.grad[4].abs().max()) == 0
    assert float((s.grad * mask[:, :, None]).abs().max()) == 0 and float((s.grad * mask[:, None, :]).abs().max()) == 0
    assert float((a.sum(1)[~mask] - 1).abs().max()) <= 1e-12
