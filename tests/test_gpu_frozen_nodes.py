"""Frozen parameters and inputs without a gradient, node by node: the branches of the backward passes that depend on `needs_input_grad`
(Linear1x1: gx / gw / gb in any combination, the side-stream form, the ResidualLink / ReluLink hand-offs; GroupNorm1: the residual's gradient;
the channels-last conv nodes, which return gradients for frozen parameters and leave it to autograd to drop them).

Every case runs the node twice on the same seeded operands - everything requiring a gradient, then a subset frozen - and asserts
  1. every frozen leaf has `.grad is None`;
  2. every gradient that exists in both runs is torch.equal (the same launches read the same operands);
  3. every gradient that exists matches the float64 torch formulation, to the tolerance of the node's all-trainable test (named at each
     group; the float64 reference is computed once per case and shared by the subsets)."""
import copy
import itertools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv import rel, relf
from test_gpu_dropout import keep_mask, drop_scale

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _leaf(t, need):
    return t.detach().clone().requires_grad_(True) if need else t.detach().clone()


def _maxerr(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.abs().max().clamp_min(1e-30))


def _check(got, full, ref, tol, bit=True):
    """got / full: name -> gradient of the frozen / the all-trainable run (None: the leaf was frozen); ref: name -> float64 gradient;
    tol(name) -> bound of _maxerr, or a callable (got, ref) -> bool"""
    seen = []
    for k, g in got.items():
        if g is None:
            continue
        assert bool(torch.isfinite(g).all()), k
        if bit:
            assert torch.equal(g, full[k]), 'gradient %s differs from the all-trainable run' % k
        t = tol(k)
        if callable(t):
            assert t(g, ref[k]), k
        else:
            seen.append('%s %.1e' % (k, _maxerr(g, ref[k])))
            assert _maxerr(g, ref[k]) <= t, (k, _maxerr(g, ref[k]), t)
    if seen:
        print('against float64 (of max):', '  '.join(seen))


# ---- K.Linear1x1 (tolerances: test_gpu_modules.test_linear1x1_exact) ---------------------------------------------------------------------
@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('N,Cin,Cout,T', [(2, 80, 96, 37), (1, 64, 256, 64)])
def test_linear1x1_every_subset(N, Cin, Cout, T, relu, bf16):
    """all seven non-empty subsets of (x, w, bias) requiring a gradient.  With the ReLU the kernel masks by ITS y > 0 (an output within
    rounding of the kink may fall on the other side than in float64, which test_linear1x1_exact sidesteps by not comparing gx / gw there):
    the float64 gradients here take the kernel's own mask, so the exact-arithmetic bounds hold for them with and without the ReLU."""
    from pytorch_sound_amd import kernels as K
    torch.manual_seed(N * 1000 + T)
    x0 = torch.randn(N, Cin, T, device=DEV)
    w0 = torch.randn(Cout, Cin, 1, device=DEV) / Cin ** 0.5
    b0 = torch.randn(Cout, device=DEV)
    g = torch.randn(N, Cout, T, device=DEV)

    def run(need):
        x, w, b = _leaf(x0, need[0]), _leaf(w0, need[1]), _leaf(b0, need[2])
        y = K.Linear1x1.apply(x, w, b, relu, bf16)
        (y * g).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), {'x': x.grad, 'w': w.grad, 'b': b.grad}

    y, full = run((True, True, True))
    rnd = (lambda t: t.to(torch.bfloat16).double()) if bf16 else (lambda t: t.double())
    xd, wd = x0.double(), w0.double().squeeze(-1)
    gd = g.double() * (y > 0) if relu else g.double()
    ref = {'x': torch.einsum('oc,not->nct', rnd(wd), rnd(gd)), 'w': torch.einsum('not,nct->oc', rnd(gd), rnd(xd)).unsqueeze(-1),
           'b': gd.sum((0, 2))}
    base = 1e-5 if bf16 else 2e-6
    tol = {'x': base, 'w': base * 4, 'b': 1e-4 if relu else base * 4}
    _check(full, full, ref, tol.get)
    for need in itertools.product([True, False], repeat=3):
        if not any(need) or all(need):
            continue
        y2, got = run(need)
        assert torch.equal(y2, y)
        for k, n in zip('xwb', need):
            assert (got[k] is None) == (not n), (need, k)
        _check(got, full, ref, tol.get)


# ---- K.GroupNorm1 (tolerances: test_gpu_modules.test_groupnorm1_vs_torch, test_gpu_dropout.test_groupnorm1_drop_vs_float64) -------------------
GN_SUBSETS = [('x',), ('res',), ('gamma', 'beta'), ('x', 'res'), ('x', 'gamma'), ('res', 'beta'), ('x', 'res', 'gamma', 'beta')]


@pytest.mark.parametrize('drop', [None, 0.1])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('N,C,T', [(3, 16, 33), (2, 32, 64)])
def test_groupnorm1_subsets(N, C, T, relu, drop):
    """(3, 16, 33): rows that no 16-byte access fits; (2, 32, 64): the 16-byte rows.  Subsets of (x, res, gamma, beta) with a residual, and
    without one (res=None).  With dropout the residual's gradient is written only when it is wanted, and x's is an exact zero where the
    element was dropped."""
    from pytorch_sound_amd import kernels as K
    torch.manual_seed(N + C)
    ops = {'x': torch.randn(N, C, T, device=DEV) * 2 + 0.7, 'res': torch.randn(N, C, T, device=DEV),
           'gamma': torch.randn(C, device=DEV) * 0.3 + 1, 'beta': torch.randn(C, device=DEV) * 0.2}
    g = torch.randn(N, C, T, device=DEV)
    seed, call = 11 + T, 3
    keep = None if drop is None else torch.from_numpy(keep_mask((N, C, T), seed, call, drop))

    def run(need, with_res=True):
        if drop is not None:
            K.dropout_seed(seed, call=call)
        t = {k: _leaf(v, k in need) for k, v in ops.items()}
        y = K.GroupNorm1.apply(t['x'], t['res'] if with_res else None, t['gamma'], t['beta'], 1e-5, relu, None, drop)
        (y * g).sum().backward()
        torch.cuda.synchronize()
        return y.detach(), {k: (v.grad if with_res or k != 'res' else None) for k, v in t.items()}

    def ref64(with_res):
        t = {k: v.double().cpu().requires_grad_(True) for k, v in ops.items()}
        xin = t['x'] if keep is None else t['x'] * (keep.double() * drop_scale(drop))
        yr = F.group_norm(xin + t['res'] if with_res else xin, 1, t['gamma'], t['beta'], 1e-5)
        yr = torch.relu(yr) if relu else yr
        (yr * g.double().cpu()).sum().backward()
        return yr.detach(), {k: v.grad for k, v in t.items()}

    for with_res in (True, False):
        names = ('x', 'res', 'gamma', 'beta') if with_res else ('x', 'gamma', 'beta')
        yr, ref = ref64(with_res)
        y, full = run(names, with_res)
        assert _maxerr(y, yr) <= 3e-6
        _check({k: full[k] for k in names}, full, ref, lambda k: 2e-5)
        for need in GN_SUBSETS:
            if not with_res:
                need = tuple(k for k in need if k != 'res')
            if not need or set(need) == set(names):
                continue
            y2, got = run(need, with_res)
            assert torch.equal(y2, y), need
            for k in ops:
                assert (got[k] is None) == (k not in need), (need, k)
            _check(got, full, ref, lambda k: 2e-5)
            if keep is not None and got['x'] is not None:
                assert bool((got['x'].cpu()[~keep] == 0).all()), 'gx is an exact zero where the element was dropped'
            if keep is not None and got['res'] is not None:
                assert float((got['res'].cpu()[~keep] != 0).float().mean()) > 0.99, 'the residual\'s gradient is not masked'


# ---- MultiHeadAttention / PointwiseFeedForward (tolerances: test_config4_block_vs_float64, test_block_under_autocast_uses_bf16_products) ----
def _modules():
    from pytorch_sound_amd.models.modules import MultiHeadAttention, PointwiseFeedForward
    torch.manual_seed(7)
    mha, ffn = MultiHeadAttention(64, 4, 0.0), PointwiseFeedForward(64, 0.0)
    with torch.no_grad():
        for m in (mha, ffn):
            m.layernorm.weight.copy_(1 + 0.2 * torch.randn(64))
            m.layernorm.bias.copy_(0.1 * torch.randn(64))
    N, T = 2, 50
    mask = torch.arange(T)[None, :] >= torch.tensor([50, 31])[:, None]                     # ragged: the second clip has 31 frames
    x0 = 0.5 * torch.randn(N, 64, T) * (~mask).unsqueeze(1)
    gy = torch.randn(N, 64, T)
    return mha, ffn, x0, mask, gy


def _run_module(mod, x0, mask, gy, need_x, frozen, autocast=False, backward=True):
    for k, p in mod.named_parameters():
        p.requires_grad_(not any(k.startswith(f) for f in frozen))
        p.grad = None
    x = _leaf(x0, need_x)
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        y = mod(x, mask) if mask is not None else mod(x)
    y = y[0] if isinstance(y, tuple) else y
    if backward:
        (y.float() * gy).sum().backward()
        torch.cuda.synchronize()
    grads = {k: p.grad for k, p in mod.named_parameters()}
    grads['x'] = x.grad
    for p in mod.parameters():
        p.requires_grad_(True)
    return y.detach(), grads


def _module_ref(mod, x0, mask, gy):
    """the same module in float64 on the host: the torch formulation the golden tests pin"""
    ref = copy.deepcopy(mod).cpu().double()
    return _run_module_host(ref, x0.cpu().double(), None if mask is None else mask.cpu(), gy.cpu().double())


def _run_module_host(ref, x0, mask, gy):
    x = x0.clone().requires_grad_(True)
    y = ref(x, mask) if mask is not None else ref(x)
    y = y[0] if isinstance(y, tuple) else y
    (y * gy).sum().backward()
    grads = {k: p.grad for k, p in ref.named_parameters()}
    grads['x'] = x.grad
    return y.detach(), grads


MHA_CASES = {'a': (False, ()), 'b': (True, ('linear_kvq',)), 'c': (True, ('linear.',)), 'd': (True, ('layernorm',)),
             'e': (True, ('linear_kvq', 'linear.', 'layernorm'))}
FFN_CASES = {'a': (False, ()), 'd': (True, ('layernorm',)), 'e': (True, ('ff.0', 'ff.2', 'layernorm')), 'f': (True, ('ff.0',)),
             'g': (True, ('ff.2',))}


@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'autocast_bf16'])
@pytest.mark.parametrize('which', ['mha', 'ffn'])
def test_transformer_nodes_frozen(which, autocast):
    """(a) input without a gradient (no ResidualLink; the feed-forward block still gets its ReluLink), (b) - (g) single projections / the
    norm's affine / everything frozen with an input that requires a gradient, (h) ff[0] frozen and no input gradient: forward only.
    fp32: 3e-5 of max on the output, 2e-4 on gradients; under autocast 3e-2 relative Frobenius."""
    mha, ffn, x0, mask, gy = _modules()
    mod, mask = (mha, mask) if which == 'mha' else (ffn, None)
    yr, ref = _module_ref(mod, x0, mask, gy)
    mod = mod.to(DEV)
    x0, gy = x0.to(DEV), gy.to(DEV)
    mask = None if mask is None else mask.to(DEV)
    frob = lambda a, b: float((a.double().cpu() - b).norm() / b.norm()) <= 3e-2          # noqa: E731
    tol = (lambda k: frob) if autocast else (lambda k: 2e-4)
    y, full = _run_module(mod, x0, mask, gy, True, (), autocast)
    assert frob(y, yr) if autocast else _maxerr(y, yr) <= 3e-5
    _check(full, full, ref, tol)
    for case, (need_x, frozen) in (MHA_CASES if which == 'mha' else FFN_CASES).items():
        y2, got = _run_module(mod, x0, mask, gy, need_x, frozen, autocast)
        assert torch.equal(y2, y), case
        for k, v in got.items():
            is_frozen = (k == 'x' and not need_x) or any(k.startswith(f) for f in frozen)
            assert (v is None) == is_frozen, (case, k)
        _check(got, full, ref, tol)
    if which == 'ffn':
        y2, got = _run_module(mod, x0, None, gy, False, ('ff.0',), autocast, backward=False)          # (h)
        assert torch.equal(y2, y) and all(v is None for v in got.values())


def test_links_hold_nothing_after_backward():
    """the feed-forward block composed by hand from _conv1x1 / _add_norm with links of this test's own: after every backward the
    ResidualLink holds no tensor, whoever was frozen.  The input gradient with the link (W^T gy + the residual's gradient in one GEMM
    epilogue, psnd_linear1x1_bwd_acc) and without it (two tensors, added by autograd) comes from different kernels: it is compared with
    float64 only (assertion 2 is dropped for this pair); parameter gradients read the same operands either way and stay torch.equal."""
    from pytorch_sound_amd import kernels as K
    import pytorch_sound_amd.models.modules as M
    _, ffn, x0, _, gy = _modules()
    _, ref = _module_ref(ffn, x0, None, gy)
    ffn, x0, gy = ffn.to(DEV), x0.to(DEV), gy.to(DEV)

    def run(need_x, frozen, linked):
        for k, p in ffn.named_parameters():
            p.requires_grad_(not any(k.startswith(f) for f in frozen))
            p.grad = None
        x = _leaf(x0, need_x)
        link = K.ResidualLink() if linked else None
        rl = K.ReluLink()
        h = M._conv1x1(ffn.ff[0], x, relu=True, link=link, relu_link=rl, hidden_out=True, pad_rows=True)
        y = M._conv1x1(ffn.ff[2], h, relu_link=rl, t_len=x.size(-1))
        out = M._add_norm(ffn.layernorm, y, x, relu=True, link=link)
        (out * gy).sum().backward()
        torch.cuda.synchronize()
        grads = {k: p.grad for k, p in ffn.named_parameters()}
        grads['x'] = x.grad
        for p in ffn.parameters():
            p.requires_grad_(True)
        return link, rl, grads

    link, rl, full = run(True, (), True)
    assert link.consumer and link.g is None and rl.consumer and not rl.masked
    _check(full, full, ref, lambda k: 2e-4)
    for need_x, frozen in [(True, ('ff.0',)), (True, ('ff.0', 'ff.2', 'layernorm')), (False, ()), (False, ('ff.0',)), (True, ('layernorm',))]:
        link, rl, got = run(need_x, frozen, True)
        assert link.g is None, 'the ResidualLink still holds a gradient'
        assert link.consumer == need_x, 'the projection registers only when it will produce a gradient for x'
        assert not rl.masked
        _check(got, full, ref, lambda k: 2e-4)
    _, _, plain = run(True, (), False)
    _check({k: v for k, v in plain.items() if k != 'x'}, full, ref, lambda k: 2e-4)
    _check({'x': plain['x']}, full, ref, lambda k: 2e-4, bit=False)


# ---- cl.fused_conv (tolerances: test_gpu_conv.test_fused_conv_fwd_bwd: 2e-2 of max on outputs, 3e-2 relative Frobenius on gradients) ----------
CONV_SUBSETS = [('x', 'res', 'v', 'b'), ('x', 'res', 'v', 'g'), ('x', 'res'), ('res', 'v', 'g', 'b'), ('x', 'v', 'g', 'b'), ('v',), ('x',)]


def _conv_runs(run, ref, names, out_tol, frozen_sets):
    """shared driver of the channels-last nodes: run(need) -> (outputs, grads by name)"""
    frob = lambda a, b: relf(a.cpu().double(), b) < 3e-2                                  # noqa: E731
    outs, full = run(names)
    for o, r in zip(outs, ref[0]):
        assert rel(o.cpu().double(), r) < out_tol
    _check(full, full, ref[1], lambda k: frob)
    for need in frozen_sets:
        outs2, got = run(need)
        assert all(torch.equal(a, b) for a, b in zip(outs, outs2)), need
        for k in names:
            assert (got[k] is None) == (k not in need), (need, k)
        _check(got, full, ref[1], lambda k: frob)


@pytest.mark.parametrize('Cin,Cout,k,dil,L,N', [(64, 64, 3, 1, 50, 2), (64, 40, 7, 3, 61, 2)])
def test_fused_conv_subsets(Cin, Cout, k, dil, L, N):
    """with a residual, raw and activated outputs; weight_g frozen, bias frozen, all three parameters frozen, x or res without a gradient"""
    from pytorch_sound_amd import cl
    from pytorch_sound_amd.models.vocoders.hifi_gan import WNConv1d
    torch.manual_seed(Cin + k)
    pad = (k * dil - dil) // 2
    conv = WNConv1d(Cin, Cout, k, dil, pad, init_std=0.05)
    with torch.no_grad():
        conv.weight_g.mul_(1.0 + 0.3 * torch.rand_like(conv.weight_g))
    x0, r0 = torch.randn(N, Cin, L), torch.randn(N, Cout, L)
    gy, gya = torch.randn(N, Cout, L), torch.randn(N, Cout, L)
    params = {'v': 'weight_v', 'g': 'weight_g', 'b': 'bias'}

    c64 = copy.deepcopy(conv).double()
    xr, rr = x0.double().requires_grad_(True), r0.double().requires_grad_(True)
    yr = c64(xr) + rr
    yar = F.leaky_relu(yr, 0.1)
    ((yr * gy.double()).sum() + (yar * gya.double()).sum()).backward()
    ref = ((yr.detach(), yar.detach()), {'x': xr.grad, 'res': rr.grad, **{s: getattr(c64, a).grad for s, a in params.items()}})

    conv = conv.to(DEV)
    x0, r0, gy, gya = (t.to(DEV) for t in (x0, r0, gy, gya))
    shape = cl.CLShape(N, L, pad + 1)

    def run(need):
        for s, a in params.items():
            getattr(conv, a).requires_grad_(s in need)
            getattr(conv, a).grad = None
        xc, rc = _leaf(x0, 'x' in need), _leaf(r0, 'res' in need)
        yb, yab = cl.fused_conv(cl.ToCL.apply(xc, shape, 0), conv, shape, cl.ToCL.apply(rc, shape, 0), True, True, 0.1)
        y2, ya2 = cl.FromCL.apply(yb, Cout, L, shape), cl.FromCL.apply(yab, Cout, L, shape)
        ((y2 * gy).sum() + (ya2 * gya).sum()).backward()
        torch.cuda.synchronize()
        return (y2.detach(), ya2.detach()), {'x': xc.grad, 'res': rc.grad, **{s: getattr(conv, a).grad for s, a in params.items()}}

    _conv_runs(run, ref, ('x', 'res', 'v', 'g', 'b'), 2e-2, CONV_SUBSETS)


# ---- cl.ConvTransposeCL (tolerances: test_gpu_config3.test_polyphase_conv_transpose_exact_on_rounded_operands) ------------------------------
@pytest.mark.parametrize('Cin,Cout,u,L,N', [(64, 32, 8, 32, 3), (16, 8, 2, 24, 1)])
def test_conv_transpose_cl_subsets(Cin, Cout, u, L, N):
    """float64 arithmetic on the bf16-rounded operands, as the all-trainable test: the bf16 input gradient to one rounding (+ 4e-4 of max),
    the fp32 parameter gradients to 2e-4 of max"""
    from pytorch_sound_amd import cl
    from pytorch_sound_amd.models.vocoders.hifi_gan import WNConvTranspose1d
    torch.manual_seed(Cin + u)
    K_, pad = 2 * u, u // 2
    up = WNConvTranspose1d(Cin, Cout, K_, u, pad, init_std=0.05).to(DEV)
    with torch.no_grad():
        up.weight_g.mul_(1.0 + 0.3 * torch.rand_like(up.weight_g))
    bf = lambda t: t.to(torch.bfloat16).double()                     # noqa: E731
    x0 = torch.randn(N, Cin, L, device=DEV)
    gy, gya = torch.randn(N, Cout, L * u, device=DEV), torch.randn(N, Cout, L * u, device=DEV)
    shape, out_shape = cl.CLShape(N, L, 3), cl.CLShape(N, L * u, 11)
    params = {'v': 'weight_v', 'g': 'weight_g', 'b': 'bias'}

    def run(need):
        for s, a in params.items():
            getattr(up, a).requires_grad_(s in need)
            getattr(up, a).grad = None
        xc = _leaf(x0, 'x' in need)
        raw, act = cl.ConvTransposeCL.apply(cl.ToCL.apply(xc, shape, 0), up.weight_v, up.weight_g, up.bias, shape, out_shape, u, pad, 0.1)
        y2, ya2 = cl.FromCL.apply(raw, Cout, L * u, out_shape), cl.FromCL.apply(act, Cout, L * u, out_shape)
        ((y2 * gy).sum() + (ya2 * gya).sum()).backward()
        torch.cuda.synchronize()                                      # the parameter side runs on its own stream
        return (y2.detach(), ya2.detach()), {'x': xc.grad, **{s: getattr(up, a).grad for s, a in params.items()}}

    (y2, ya2), full = run(('x', 'v', 'g', 'b'))
    v32, g32 = up.weight_v.detach(), up.weight_g.detach()
    w32 = v32 * (g32 / v32.flatten(1).norm(dim=1).view(-1, 1, 1))
    wq, xq = bf(w32), bf(x0)
    v = F.conv_transpose1d(xq, wq, up.bias.detach().double(), u, pad)
    ulp = 2.0 ** -8
    tol_bf = lambda got, want: bool(((got.double() - want).abs() <= 1.01 * ulp * want.abs() + 4e-4 * float(want.abs().max())).all())  # noqa: E731
    assert tol_bf(y2, v) and tol_bf(ya2, F.leaky_relu(v, 0.1))
    gcomb = bf(gy.to(torch.bfloat16).float() + gya.to(torch.bfloat16).float() * torch.where(ya2 > 0, 1.0, 0.1).float())
    v64, g64, b64 = (t.detach().double().requires_grad_(True) for t in (v32, g32, up.bias))
    w64 = v64 * (g64 / v64.flatten(1).norm(dim=1).view(-1, 1, 1))
    wq_leaf = wq.clone().requires_grad_(True)                        # the kernels see bf16(w): gradient at the rounded point, chained through the exact norm
    (F.conv_transpose1d(xq, wq_leaf, b64, u, pad) * gcomb).sum().backward()
    w64.backward(wq_leaf.grad)
    ref = {'x': F.conv1d(gcomb, wq, None, u, pad), 'v': v64.grad, 'g': g64.grad, 'b': b64.grad}
    tol = lambda k: tol_bf if k == 'x' else 2e-4                    # noqa: E731
    _check(full, full, ref, tol)
    for need in [('x', 'v', 'b'), ('x', 'v', 'g'), ('x',), ('v', 'g', 'b'), ('g',), ('x', 'b')]:
        outs, got = run(need)
        assert torch.equal(outs[0], y2) and torch.equal(outs[1], ya2), need
        for k in ('x', 'v', 'g', 'b'):
            assert (got[k] is None) == (k not in need), (need, k)
        _check(got, full, ref, tol)


# ---- cl.resblock1_cl and whole models (tolerances: test_gpu_hifigan.test_generator_cl_matches_torch_path, which holds the resblocks of a
# generator to them: output 4e-2, the input gradient and all parameter gradients together 8e-2 relative Frobenius, the worst single tensor
# 0.3; the block alone: output 2e-2 of max as test_wide_tap_pair_launch_matches_two_launches; separator: test_separator_cl_matches_torch_path) ---
def _model_case(named, run, ref, cases, out_tol, single_tol, together_tol=None, out_err=relf, x_leaf=True):
    """named: name -> parameter; run(need_x) -> (output, x.grad or None) after a backward; ref: (output, name -> float64 gradient, 'x' incl.);
    x_leaf False: the model's input never carries a gradient"""
    def one(need_x, frozen):
        need_x = need_x and x_leaf
        for k, p in named.items():
            p.requires_grad_(not any(k.startswith(f) for f in frozen))
            p.grad = None
        out, gx = run(need_x)
        torch.cuda.synchronize()
        got = {k: p.grad for k, p in named.items()}
        got['x'] = gx
        for k, v in got.items():
            is_frozen = (k == 'x' and not need_x) or any(k.startswith(f) for f in frozen)
            assert (v is None) == is_frozen, (frozen, k)
        for p in named.values():
            p.requires_grad_(True)
        return out, got

    def against_ref(got):
        have = [k for k, v in got.items() if v is not None and k != 'x' and float(ref[1][k].norm()) > 0]
        errs = {k: relf(got[k].cpu().double(), ref[1][k]) for k in have}
        if errs:
            print('worst single gradient %s %.1e (bound %.0e)' % (max(errs, key=errs.get), max(errs.values()), single_tol))
        for k in have:
            assert errs[k] <= single_tol, (k, errs[k])
        if together_tol is not None and have:
            a, b = torch.cat([got[k].flatten().cpu().double() for k in have]), torch.cat([ref[1][k].flatten() for k in have])
            print('all parameter gradients together %.1e (bound %.0e)' % (relf(a, b), together_tol))
            assert relf(a, b) <= together_tol
        if got['x'] is not None:
            assert relf(got['x'].cpu().double(), ref[1]['x']) <= (together_tol or single_tol)

    out, full = one(True, ())
    assert out_err(out.cpu().double(), ref[0]) <= out_tol
    against_ref(full)
    for need_x, frozen in cases:
        out2, got = one(need_x, frozen)
        assert torch.equal(out2, out), frozen
        for k, v in got.items():
            if v is not None:
                assert torch.equal(v, full[k]), (frozen, k)
        against_ref(got)


@pytest.mark.parametrize('chain', ['3', '0'], ids=['chain', 'pair_backward'])
def test_resblock1_cl_frozen(chain, monkeypatch):
    """64 channels, k = 3, dilations (1, 3, 5), T = 50, N = 2: convs1[1] wholly frozen, every weight_g, every bias, the input without a
    gradient; PSND_CL_CHAIN=0: one pair launch per pair in the backward instead of the chain launch"""
    from pytorch_sound_amd import cl
    from pytorch_sound_amd.models.vocoders.hifi_gan import ResBlock1
    monkeypatch.setenv('PSND_CL_CHAIN', chain)
    torch.manual_seed(64 + 9)
    C, T, N = 64, 50, 2
    blk = ResBlock1(None, C, 3, (1, 3, 5))
    with torch.no_grad():
        for c in list(blk.convs1) + list(blk.convs2):
            c.weight_g.copy_(0.7 + 0.6 * torch.rand_like(c.weight_g))
    x0, gy = torch.randn(N, C, T), torch.randn(N, C, T)
    b64 = copy.deepcopy(blk).double()
    xr = x0.double().requires_grad_(True)
    yr = b64(xr)
    (yr * gy.double()).sum().backward()
    ref = (yr.detach(), {**{k: p.grad for k, p in b64.named_parameters()}, 'x': xr.grad})
    blk, x0, gy = blk.to(DEV), x0.to(DEV), gy.to(DEV)
    shape = cl.CLShape(N, T, 25)

    def run(need_x):
        xc = _leaf(x0, need_x)
        xr_ = cl.ToCL.apply(xc, shape, 0)
        y, _ = cl.resblock1_cl(blk, xr_, cl.MeanActCL.apply(0.1, xr_), shape, want_raw=True)
        out = cl.FromCL.apply(y, C, T, shape)
        (out * gy).sum().backward()
        return out.detach(), xc.grad

    names = [k for k, _ in blk.named_parameters()]
    cases = [(True, ('convs1.1.',)), (True, tuple(k for k in names if k.endswith('weight_g'))),
             (True, tuple(k for k in names if k.endswith('bias'))), (False, ())]
    _model_case(dict(blk.named_parameters()), run, ref, cases, 2e-2, 0.3, 8e-2, out_err=rel)


@pytest.mark.parametrize('frozen', ['conv_pre', 'blocks.0', 'conv_post'])
def test_separator_frozen(frozen):
    """build_model('conv_separator_voicebank', channels 64, two blocks) on a (2, 513, 40) magnitude: the head conv (the chain's input needs
    no gradient: its input-gradient role is skipped), a whole block, the tail conv frozen.  2e-2 of max on the estimate, 5e-2 relative
    Frobenius on every parameter gradient."""
    from pytorch_sound_amd.models import build_model
    from pytorch_sound_amd.models import separator  # noqa: F401
    torch.manual_seed(0)
    model = build_model('conv_separator_voicebank', {'channels': 64, 'num_blocks': 2})
    mag, tgt = torch.rand(2, 513, 40) * 4, torch.rand(2, 513, 40)
    m64 = copy.deepcopy(model).double()
    est = m64._forward_plain(mag.double())
    (est - tgt.double()).abs().mean().backward()
    ref = (est.detach(), {k: p.grad for k, p in m64.named_parameters()})
    model, mag, tgt = model.to(DEV), mag.to(DEV), tgt.to(DEV)

    def run(need_x):
        out = model(mag)
        (out - tgt).abs().mean().backward()
        return out.detach().float(), None

    _model_case(dict(model.named_parameters()), run, (ref[0], {**ref[1], 'x': None}), [(False, (frozen + '.',))], 2e-2, 5e-2, out_err=rel,
                x_leaf=False)


@pytest.mark.parametrize('upsample', ['polyphase', 'kernel'])
def test_hifigan_ups_frozen(upsample):
    """the tiny HiFi-GAN of test_gpu_hifigan.py on (2, 80, 12) with every upsampler frozen, for both cl_upsample modes"""
    from test_gpu_hifigan import _make
    g = _make('2', [4, 4], [8, 8], 64, [3, 5], [[1, 2], [2, 6]])
    g.cl_upsample = upsample
    torch.manual_seed(11)
    x0 = torch.randn(2, 80, 12, device=DEV)
    assert g._cl_ok(x0)
    g64 = copy.deepcopy(g).cpu().double()
    g64.use_cl = False
    xr = x0.cpu().double().requires_grad_(True)
    yr = g64(xr)
    w = torch.randn(yr.shape)
    (yr * w.double()).sum().backward()
    ref = (yr.detach(), {**{k: p.grad for k, p in g64.named_parameters()}, 'x': xr.grad})
    w = w.to(DEV)

    def run(need_x):
        xc = _leaf(x0, need_x)
        out = g(xc)
        (out * w).sum().backward()
        return out.detach(), xc.grad

    _model_case(dict(g.named_parameters()), run, ref, [(True, ('ups.',)), (False, ('ups.',))], 4e-2, 0.3, 8e-2)
