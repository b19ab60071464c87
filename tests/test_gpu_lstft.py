"""LearnableSTFT on HIP tensors (psnd_lstft_*: strided-view analysis, polyphase synthesis, slab basis gradient): no library path,
the reference golden and the module's own float64 CPU path as yardsticks (the bounds of tests/test_filters_golden.py
::test_learnable_stft_matches_reference), the operator identities the two backward passes rely on, no unfolded frames in memory,
bit-reproducible, capturable, frozen / mixed / other-dtype cases."""
import copy
import os
from contextlib import contextmanager

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu

# tests/test_gpu_no_library_paths.py's list + the ops an unfolded-frames formulation would use
FORBIDDEN = ('aten.bmm', 'aten.baddbmm', 'aten.mm.', 'aten.addmm', 'aten._softmax', 'aten.native_group_norm', 'aten.convolution',
             'aten.miopen', 'aten.cudnn', 'aten._fft', 'aten.stft', 'aten.istft', 'aten.im2col', 'aten.col2im', 'aten.unfold')


class _Forbid(TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if any(name.startswith(f) for f in FORBIDDEN):
            flat = torch.utils._pytree.tree_leaves((args, kwargs or {}))
            if any(isinstance(a, torch.Tensor) and a.is_cuda for a in flat):
                raise AssertionError('library op %s reached with a HIP tensor' % name)
        return func(*args, **(kwargs or {}))


@contextmanager
def forbid_library_ops():
    with _Forbid():
        yield


def _dev():
    assert torch.cuda.is_available(), 'GPU test run without a GPU'
    return torch.device('cuda:0')


def _module(n, hop, win=None, seed=0, perturb=True, **kw):
    """a LearnableSTFT whose bases are no longer a DFT (seeded noise on both)"""
    from pytorch_sound_amd.models.transforms import LearnableSTFT
    m = LearnableSTFT(n, hop, win, **kw)
    if perturb:
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            m.forward_basis.add_(0.05 * torch.randn(m.forward_basis.shape, generator=g))
            m.inverse_basis.add_(0.05 / n * torch.randn(m.inverse_basis.shape, generator=g))
    return m


def _step(m, wav):
    """transform -> inverse -> loss -> backward; everything a comparison needs, detached"""
    for p in m.parameters():
        p.grad = None
    x = wav.detach().clone().requires_grad_(True)
    mag, phase = m.transform(x)
    rec = m.inverse(mag, phase)
    (mag.sum() + rec.pow(2).sum()).backward()
    out = dict(mag=mag.detach(), phase=phase.detach(), rec=rec.detach(), gwav=x.grad)
    for name in ('forward_basis', 'inverse_basis'):
        p = getattr(m, name)
        out['g_' + name] = p.grad if isinstance(p, torch.nn.Parameter) else None
    return out


def _close(name, got, want, rel):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, '%s: shape %s vs %s' % (name, tuple(got.shape), tuple(want.shape))
    err, ref = (got - want).abs().max().item(), max(want.abs().max().item(), 1e-6)
    print('%s: max err %.3e of max %.3e (bound %.1e)' % (name, err, ref, rel))
    assert err < rel * ref, '%s: max err %.3e > %.1e * %.3e' % (name, err, rel, ref)


def _phase_close(got, want, mag, min_keep=None):
    got, want, mag = got.double().cpu().numpy(), want.double().cpu().numpy(), mag.double().cpu().numpy()
    strong = mag > 1e-3 * mag.max()
    d = np.angle(np.exp(1j * (got - want)))
    print('phase: max err %.3e rad on %.4f of the bins' % (np.abs(d[strong]).max(), strong.mean()))
    if min_keep is not None:
        assert strong.mean() >= min_keep, 'the 1e-3 * max mask keeps %.4f of the bins only: a bad test input' % strong.mean()
    assert np.abs(d[strong]).max() < 1e-3


# ---- 1. no library path ----------------------------------------------------------------------------------------------------------
def test_no_library_op_is_reached():
    dev = _dev()
    torch.manual_seed(0)
    m = _module(1024, 256, perturb=False).to(dev)
    assert isinstance(m.forward_basis, torch.nn.Parameter) and isinstance(m.inverse_basis, torch.nn.Parameter)
    wav = (0.1 * torch.randn(3, 8000, device=dev)).requires_grad_(True)
    with forbid_library_ops():
        mag, phase = m.transform(wav)
        rec = m.inverse(mag, phase)
        (mag.sum() + rec.pow(2).sum()).backward()
    torch.cuda.synchronize()
    assert mag.shape == (3, 513, 32) and phase.shape == mag.shape and rec.shape == (3, 31 * 256) and not phase.requires_grad
    for t in (wav.grad, m.forward_basis.grad, m.inverse_basis.grad):
        assert t is not None and torch.isfinite(t).all() and t.abs().max() > 0


# ---- 2. the reference golden -----------------------------------------------------------------------------------------------------
def test_matches_reference_golden_on_gpu():
    from pytorch_sound_amd.models.transforms import LearnableSTFT
    dev = _dev()
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'lstft.npz'))
    m = LearnableSTFT(256, 64, 200).to(dev)
    assert sorted(m.state_dict().keys()) == list(g['state_keys'])
    o = _step(m, torch.from_numpy(g['wav']).to(dev))
    _close('mag', o['mag'], torch.from_numpy(g['mag']), 2e-5)
    _phase_close(o['phase'], torch.from_numpy(g['phase']), torch.from_numpy(g['mag']))
    _close('rec', o['rec'], torch.from_numpy(g['rec']), 1e-4)
    rows = [0, 1, 64, 129, 200, 257]
    _close('g_forward_basis rows', o['g_forward_basis'][rows], torch.from_numpy(g['g_forward_basis_rows']), 1e-3)
    _close('g_inverse_basis rows', o['g_inverse_basis'][rows], torch.from_numpy(g['g_inverse_basis_rows']), 1e-3)


# ---- 3. float64 CPU path of the module, trained bases ----------------------------------------------------------------------------
@pytest.mark.parametrize('n,hop,win,N,T', [
    (256, 64, 200, 3, 2048),
    (400, 160, None, 2, 4000),
    (1024, 256, None, 2, 32000),
    (150, 37, 101, 3, 1999),         # hop does not divide n, odd tile edges
    (255, 50, None, 2, 3000),        # n odd: no Nyquist row
    (256, 64, None, 1, 5000),        # one clip
    (256, 64, None, 2, 129),         # F = 3 ... and the shortest clips below
    (256, 100, None, 2, 130),        # F = 2
    (512, 16, None, 2, 3000),        # 32 taps per phase
])
def test_matches_float64_path_with_trained_bases(n, hop, win, N, T):
    dev = _dev()
    m = _module(n, hop, win, seed=n + hop)
    wav = 0.1 * torch.randn(N, T, generator=torch.Generator().manual_seed(T))
    want = _step(copy.deepcopy(m).double(), wav.double())
    got = _step(m.to(dev), wav.to(dev))
    _close('mag', got['mag'], want['mag'], 2e-5)
    _phase_close(got['phase'], want['phase'], want['mag'], min_keep=0.99)
    _close('rec', got['rec'], want['rec'], 1e-4)
    _close('g_forward_basis', got['g_forward_basis'], want['g_forward_basis'], 1e-3)
    _close('g_inverse_basis', got['g_inverse_basis'], want['g_inverse_basis'], 1e-3)
    _close('gwav', got['gwav'], want['gwav'], 1e-3)


# ---- 4. operator identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,n,hop,N,F,tail', [(258, 256, 64, 3, 29, 0), (152, 150, 37, 2, 51, 11), (1026, 1024, 256, 2, 9, 0),
                                              (7, 33, 5, 1, 1, 0), (40, 64, 200, 2, 4, 3)])
def test_synthesis_is_conv_transpose_and_adjoint_of_analysis(C, n, hop, N, F, tail):
    from pytorch_sound_amd import kernels as K
    dev = _dev()
    gen = torch.Generator().manual_seed(C + hop)
    B, w = torch.randn(C, n, generator=gen) / n ** 0.5, torch.rand(n, generator=gen) + 0.1
    g = torch.randn(N, C, F, generator=gen)
    L = n + hop * (F - 1)
    mult = torch.rand(L + tail, generator=gen) + 0.5
    want = torch.nn.functional.conv_transpose1d(g.double(), (B.double() * w.double())[:, None, :], stride=hop).squeeze(1)
    y = K.lstft_synthesis(g.to(dev), B.to(dev), w.to(dev), hop, length=L + tail)
    assert y.shape == (N, L + tail) and (tail == 0 or y[:, L:].abs().max().item() == 0.0)      # samples behind the last frame: zeros
    _close('synthesis', y[:, :L], want, 2e-5)
    ym = K.lstft_synthesis(g.to(dev), B.to(dev), w.to(dev), hop, mult=mult.to(dev), length=L + tail)
    _close('synthesis * mult', ym[:, :L], want * mult[:L].double(), 2e-5)
    # <A(x), g> = <x, S(g)> with the same basis: what the two backward passes rely on
    x = torch.randn(N, L + tail, generator=gen)
    spec = K.lstft_analysis(x.to(dev), B.to(dev), w.to(dev), hop)
    assert spec.shape == (N, C, (L + tail - n) // hop + 1)
    spec = spec[:, :, :F]
    want_spec = torch.nn.functional.conv1d(x.double()[:, None], (B.double() * w.double())[:, None, :], stride=hop)[:, :, :F]
    _close('analysis', spec, want_spec, 2e-5)
    lhs, rhs = (spec.double().cpu() * g.double()).sum().item(), (x.double() * y.double().cpu()).sum().item()
    scale = (spec.double().cpu() * g.double()).abs().sum().item()
    print('adjoint: %.9e vs %.9e (sum of magnitudes %.3e)' % (lhs, rhs, scale))
    assert abs(lhs - rhs) <= 1e-5 * scale                            # fp32 round-off of either side, far below any wrong tap
    # the basis gradient against float64
    gb = K.lstft_basis_grad(g.to(dev), x.to(dev), w.to(dev), hop, B)
    fr = x.double().unfold(1, n, hop)[:, :F]                          # CPU float64: (N, F, n)
    _close('basis gradient', gb, torch.einsum('zcf,zfm->cm', g.double(), fr) * w.double(), 2e-5)


# ---- 5. no unfolded frames -------------------------------------------------------------------------------------------------------
def test_transform_never_materialises_frames():
    dev = _dev()
    N, T, n, hop = 8, 65536, 1024, 64
    m = _module(n, hop, perturb=False).to(dev)
    wav = 0.1 * torch.randn(N, T, device=dev)
    with torch.no_grad():
        m.transform(wav[:, :4096])                                   # first-call work (library load) outside the measurement
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        mag, phase = m.transform(wav)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    F = T // hop + 1
    assert mag.shape == (N, n // 2 + 1, F)
    nbytes = lambda *shape: 4 * int(np.prod(shape))                  # noqa: E731
    bound = 2 * nbytes(N, n // 2 + 1, F) + nbytes(N, n + 2, F) + 2 * nbytes(N, T + n) + (1 << 20)
    print('peak %.1f MB, bound %.1f MB, frames would be %.1f MB' % (peak / 1e6, bound / 1e6, nbytes(N, n, F) / 1e6))
    assert peak <= bound


# ---- 6. reproducible -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,hop,N,T', [(1024, 256, 8, 32000), (256, 64, 32, 16000), (150, 37, 3, 1999)])
def test_same_bits_from_run_to_run(n, hop, N, T):
    dev = _dev()
    m = _module(n, hop, seed=1).to(dev)
    wav = 0.1 * torch.randn(N, T, device=dev)
    runs = []
    for _ in range(3):
        o = _step(m, wav)
        torch.cuda.synchronize()
        runs.append([o[k].clone() for k in ('mag', 'rec', 'gwav', 'g_forward_basis', 'g_inverse_basis', 'phase')])
    for other in runs[1:]:
        for u, v in zip(runs[0], other):
            assert torch.equal(u, v)


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------
def test_forward_backward_captured_in_a_graph_replays_the_eager_bits():
    dev = _dev()
    m = _module(256, 64, seed=2).to(dev)
    wav = (0.1 * torch.randn(4, 4000, device=dev)).requires_grad_(True)
    tgt_mag, tgt = torch.rand(4, 129, 63, device=dev), 0.1 * torch.randn(4, 62 * 64, device=dev)

    def step():
        mag, phase = m.transform(wav)
        rec = m.inverse(mag, phase)
        loss = (mag - tgt_mag).abs().mean() + (rec - tgt).pow(2).mean()
        loss.backward()
        return loss

    def grads():
        return [wav.grad, m.forward_basis.grad, m.inverse_basis.grad]

    def clear():
        for t in [wav] + list(m.parameters()):
            t.grad = None

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            clear()
            eager_loss = step().detach().clone()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = [g.clone() for g in grads()]
    clear()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = step()
    static = grads()
    for g in static:
        g.zero_()
    loss.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss, eager_loss)
    for u, v in zip(static, eager):
        assert u.abs().max() > 0 and torch.equal(u, v)


# ---- 8. frozen, mixed, other dtypes, short clips ---------------------------------------------------------------------------------
def test_frozen_and_mixed_modules():
    dev = _dev()
    wav = 0.1 * torch.randn(2, 3000, device=dev)
    ref = _step(_module(256, 64, perturb=False).to(dev), wav)
    frozen = _module(256, 64, perturb=False, trainable_forward=False, trainable_inverse=False).to(dev)
    assert not list(frozen.parameters()) and len(frozen.state_dict()) == 3
    o = _step(frozen, wav)
    for k in ('mag', 'phase', 'rec', 'gwav'):
        assert torch.equal(o[k], ref[k])
    fwd_only = _module(256, 64, perturb=False, trainable_inverse=False).to(dev)
    o = _step(fwd_only, wav)
    assert [k for k, _ in fwd_only.named_parameters()] == ['forward_basis'] and torch.equal(o['g_forward_basis'], ref['g_forward_basis'])
    inv_only = _module(256, 64, perturb=False, trainable_forward=False).to(dev)
    o = _step(inv_only, wav)
    assert [k for k, _ in inv_only.named_parameters()] == ['inverse_basis'] and torch.equal(o['g_inverse_basis'], ref['g_inverse_basis'])
    # a trainable module whose waveform needs no gradient, under no_grad, and with a frozen parameter
    m = _module(256, 64, perturb=False).to(dev)
    m.inverse_basis.requires_grad_(False)
    mag, phase = m.transform(wav)
    m.inverse(mag, phase).pow(2).sum().backward()
    assert m.inverse_basis.grad is None and m.forward_basis.grad is not None
    with torch.no_grad():
        mag2, _ = m.transform(wav)
    assert torch.equal(mag2, ref['mag'])


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16, torch.float64])
def test_other_dtypes_are_cast_in_and_out(dtype):
    dev = _dev()
    m = _module(256, 64).to(dev)
    wav32 = (0.1 * torch.randn(2, 3000, device=dev)).to(dtype).float()           # representable in `dtype`
    with forbid_library_ops():
        mag32, ph32 = m.transform(wav32)
        mag, ph = m.transform(wav32.to(dtype))
        rec = m.inverse(mag, ph)
        rec32 = m.inverse(mag.float(), ph.float())
        with torch.autocast('cuda', dtype=torch.bfloat16):                        # autocast: the same fp32 path
            mag_ac, _ = m.transform(wav32)
    assert mag.dtype == dtype and ph.dtype == dtype and rec.dtype == dtype
    assert torch.equal(mag, mag32.to(dtype)) and torch.equal(ph, ph32.to(dtype)) and torch.equal(rec, rec32.to(dtype))
    assert mag_ac.dtype == torch.float32 and torch.equal(mag_ac, mag32)
    x = wav32.to(dtype).requires_grad_(True)
    mag, ph = m.transform(x)
    m.inverse(mag, ph).float().pow(2).sum().backward()
    assert x.grad.dtype == dtype and torch.isfinite(x.grad.float()).all() and m.forward_basis.grad.dtype == torch.float32


def test_short_waveform_raises_what_reflect_padding_raises():
    dev = _dev()
    m = _module(256, 64, perturb=False)
    short = torch.zeros(2, m.pad_amount)
    with pytest.raises(RuntimeError) as cpu:
        m.transform(short)
    with pytest.raises(RuntimeError) as hip:
        copy.deepcopy(m).to(dev).transform(short.to(dev))
    assert type(hip.value) is type(cpu.value) and 'Padding size should be less than' in str(cpu.value)
    assert 'Padding size should be less than' in str(hip.value)
    mag, _ = m.to(dev).transform(torch.zeros(2, m.pad_amount + 1, device=dev))     # the shortest clip the padding takes
    assert mag.shape == (2, 129, 1 + (m.pad_amount + 1) // 64)


def test_missing_library_raises(monkeypatch):
    from pytorch_sound_amd import _lib
    dev = _dev()
    m = _module(256, 64, perturb=False).to(dev)

    def gone():
        raise _lib.PsndError('libpsnd_hip.so not found')
    monkeypatch.setattr('pytorch_sound_amd._lib.lib', gone)         # the one loader every launch goes through (_lib.on)
    with pytest.raises(_lib.PsndError):
        m.transform(torch.zeros(1, 1000, device=dev))
