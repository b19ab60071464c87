"""Masked inverse STFT on (re, im) on HIP tensors: psnd_istft_reim / psnd_istft_reim_mr / psnd_istft_reim_bwd behind kernels.istft_reim,
STFT / STFTTorchAudio.inverse_complex and ConvSeparator.separate.

The yardstick everywhere is float64 torch.istft(torch.complex(m re, m im), n_fft, hop, n_fft, window) and its autograd on the CPU.
Tolerances are the project's own for psnd_istft: forward 5e-6 max(|ref|, 1) at powers of two (test_gpu_features.py) and 2e-5 of the maximum
at the mixed-radix sizes (test_gpu_stft_anysize.py); gradients 1e-4 of the largest entry of each gradient (test_gpu_stft_modules.py), 5e-5
at the mixed-radix sizes.  eps = 1e-9 against torch.istft's plain division changes a sample by 1e-9 / env relative - the envelope inside
the kept range is of order one at every geometry here - three orders below the bound.  Every figure is printed before it is asserted
(`pytest -s`)."""
import functools
import gc
import tempfile

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import poison
from oracle import features as ofe

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 3
NONE, LINEAR, SIGMOID = 0, 1, 2

# (n_fft, hop, win_length, kernel family, frames per tile)
GEOMS = [(256, 64, None, 'tiled<16,8>', 32),
         (512, 128, None, 'span', 32),
         (512, 125, None, 'tiled<16,16>', 32),
         (1024, 256, None, 'span', 16),
         (1024, 256, 800, 'span', 16),
         (1024, 512, None, 'tiled<32,16>', 16),
         (2048, 512, None, 'tiled<32,32>', 16),
         (128, 32, None, 'generic', 1),
         (4096, 1024, None, 'generic', 1),
         (240, 60, 200, 'mixed-radix', 8),
         (400, 100, None, 'mixed-radix', 8),
         (1200, 300, None, 'mixed-radix', 8)]
# frame counts at the tile edges: one tile with a ragged end, exactly full, one over, several tiles
CASES = [(n, h, w, fam, F) for (n, h, w, fam, ft) in GEOMS for F in ((2, 32, 33, 67) if ft == 32 else (2, 16, 17, 35))]
# The generic kernel adds the <= n / hop frames of a sample with float atomics in no fixed order: two runs agree bit for bit only where a
# sample has at most two addends (they commute).  The bit-identity check therefore skips the generic sizes of the table and runs on the
# generic kernel at hop = n / 2 instead.
CASES.append((128, 64, None, 'generic, two frames per sample', 17))
IDS = ['%d-%d-%s-F%d' % (n, h, w, F) for (n, h, w, fam, F) in CASES]


def _is_mr(n):
    return n & (n - 1) != 0


@functools.lru_cache(maxsize=None)
def _plan(n, win):
    from pytorch_sound_amd import kernels as K
    return K.stft_plan(n, ofe.analysis_window(n, win)).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(n, hop, win, F):
    """seeded unit-scale spectra (nonzero im at DC and Nyquist), a linear mask with negative and exactly zero entries, logits with +-30,
    an output gradient; shared and read-only"""
    g = torch.Generator().manual_seed(n * 131 + hop * 7 + F)
    K = n // 2 + 1
    re, im = torch.randn(N, K, F, generator=g), torch.randn(N, K, F, generator=g)
    lin = torch.randn(N, K, F, generator=g)
    lin[0, 0, 0], lin[1, K - 1, F - 1], lin[2, K // 2, F // 2], lin[0, 1, :] = 0.0, 0.0, 0.0, 0.0
    lin[1, 5, 0] = -2.5
    logit = torch.randn(N, K, F, generator=g) * 3
    logit[0, 2, 0], logit[1, K - 2, F - 1], logit[2, 0, 1], logit[0, K - 1, 0] = 30.0, -30.0, 30.0, -30.0
    gout = torch.randn(N, (F - 1) * hop, generator=g)
    window = torch.from_numpy(ofe.analysis_window(n, win))
    return dict(re=re, im=im, mask={NONE: None, LINEAR: lin, SIGMOID: logit}, gout=gout, window=window)


def _yardstick(re, im, mask, kind, n, hop, window):
    re, im = re.double(), im.double()
    if kind != NONE:
        m = torch.sigmoid(mask.double()) if kind == SIGMOID else mask.double()
        re, im = m * re, m * im
    return torch.istft(torch.complex(re, im), n, hop, n, window.double())


@functools.lru_cache(maxsize=None)
def _reference(n, hop, win, F, kind):
    """float64 forward and gradients of one case and mask kind, computed once"""
    c = _inputs(n, hop, win, F)
    leaves = [c['re'].double().clone().requires_grad_(True), c['im'].double().clone().requires_grad_(True)]
    if kind != NONE:
        leaves.append(c['mask'][kind].double().clone().requires_grad_(True))
    out = _yardstick(leaves[0], leaves[1], leaves[2] if kind != NONE else None, kind, n, hop, c['window'])
    grads = torch.autograd.grad((out * c['gout'].double()).sum(), leaves)
    return out.detach(), [g.detach() for g in grads]


def _fwd_bound(n, ref):
    return 2e-5 * float(ref.abs().max()) if _is_mr(n) else 5e-6 * max(float(ref.abs().max()), 1.0)


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize('n,hop,win,fam,F', CASES, ids=IDS)
def test_forward_and_backward_against_float64(n, hop, win, fam, F):
    from pytorch_sound_amd import kernels as K
    c = _inputs(n, hop, win, F)
    plan = _plan(n, win)
    re, im = _dev(c['re']), _dev(c['im'])
    for kind in (NONE, LINEAR, SIGMOID):
        ref, gref = _reference(n, hop, win, F, kind)
        mask = _dev(c['mask'][kind])
        for eps in (0.0, 1e-9):
            got = K.istft_reim(re, im, mask, kind, n, hop, plan, eps).cpu()
            assert got.shape == ref.shape == (N, (F - 1) * hop)
            err, bound = float((got.double() - ref).abs().max()), _fwd_bound(n, ref)
            print('%s n=%d hop=%d F=%d kind=%d eps=%g: forward err %.3e (bound %.3e)' % (fam, n, hop, F, kind, eps, err, bound))
            assert err <= bound

        # backward, full call: g_re, g_im (and g_mask)
        leaves = [re.clone().requires_grad_(True), im.clone().requires_grad_(True)]
        if kind != NONE:
            leaves.append(mask.clone().requires_grad_(True))
        eps = 1e-9 if kind == LINEAR else 0.0
        out = K.istft_reim(leaves[0], leaves[1], leaves[2] if kind != NONE else None, kind, n, hop, plan, eps)
        out.backward(_dev(c['gout']))
        rel = 5e-5 if _is_mr(n) else 1e-4
        for name, leaf, gr in zip(('g_re', 'g_im', 'g_mask'), leaves, gref):
            got = leaf.grad.cpu()
            assert bool(torch.isfinite(got).all()), name
            err, top = float((got.double() - gr).abs().max()), float(gr.abs().max())
            print('    kind=%d %s err %.3e of max %.3e (%.2e)' % (kind, name, err, top, err / top))
            assert err <= rel * top, name
        g_im = leaves[1].grad
        assert bool((g_im[:, 0] == 0).all()) and bool((g_im[:, -1] == 0).all())       # exactly zero at DC and Nyquist

        # the mask-only call: re and im carry no gradient
        if kind != NONE:
            m2 = mask.clone().requires_grad_(True)
            K.istft_reim(re, im, m2, kind, n, hop, plan, eps).backward(_dev(c['gout']))
            assert torch.equal(m2.grad, leaves[2].grad)


@pytest.mark.parametrize('n,hop,win,fam,F', [c for c in CASES if c[3] != 'generic'], ids=[i for i, c in zip(IDS, CASES) if c[3] != 'generic'])
def test_dc_and_nyquist_imaginary_parts_do_not_reach_the_signal(n, hop, win, fam, F):
    from pytorch_sound_amd import kernels as K
    c = _inputs(n, hop, win, F)
    plan = _plan(n, win)
    re, im, mask = _dev(c['re']), _dev(c['im']), _dev(c['mask'][SIGMOID])
    a = K.istft_reim(re, im, mask, SIGMOID, n, hop, plan, 0.0)
    im2 = im.clone()
    im2[:, 0] = 7.0
    im2[:, -1] = -3.0
    b = K.istft_reim(re, im2, mask, SIGMOID, n, hop, plan, 0.0)
    assert poison.same_bits(a.cpu(), b.cpu())


_BANNED = ('mul', 'div', 'add', 'sub', 'where', 'cos', 'sin', 'atan2', 'sqrt', 'sigmoid', 'constant_pad_nd', 'polar')


class _ComputeOnHip(AssertionError):
    pass


class _NoAtenCompute(TorchDispatchMode):
    """raises when one of the ops IStft.backward is written in receives a HIP tensor"""

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = func.overloadpacket.__name__.rstrip('_')
        if func.namespace == 'aten' and name in _BANNED:
            flat = list(args) + list(kwargs.values())
            flat = [x for a in flat for x in (a if isinstance(a, (list, tuple)) else [a])]
            if any(isinstance(x, torch.Tensor) and x.is_cuda for x in flat):
                raise _ComputeOnHip('ATen compute op %s on a HIP tensor' % func)
        return func(*args, **kwargs)


@pytest.mark.parametrize('n,hop', [(1024, 256), (400, 100)])
def test_no_aten_compute_touches_a_hip_tensor(n, hop):
    from pytorch_sound_amd import kernels as K
    F = 17
    c = _inputs(n, hop, None, F)
    plan = _plan(n, None)
    gout = _dev(c['gout'])
    with _NoAtenCompute():
        with pytest.raises(_ComputeOnHip):                                          # the mode sees HIP tensors
            _dev(c['re']) * 2.0
        for kind in (NONE, LINEAR, SIGMOID):
            leaves = [_dev(c['re']).requires_grad_(True), _dev(c['im']).requires_grad_(True)]
            mask = None if kind == NONE else _dev(c['mask'][kind]).requires_grad_(True)
            K.istft_reim(leaves[0], leaves[1], mask, kind, n, hop, plan, 1e-9).backward(gout)
            assert leaves[0].grad is not None and (mask is None or mask.grad is not None)
        m2 = _dev(c['mask'][SIGMOID]).requires_grad_(True)                          # the typical call: the mask alone
        K.istft_reim(_dev(c['re']), _dev(c['im']), m2, SIGMOID, n, hop, plan, 1e-9).backward(gout)
        assert m2.grad is not None


@pytest.mark.parametrize('n,hop', [(1024, 256), (400, 100)])
def test_forward_and_backward_do_not_depend_on_freed_memory(n, hop):
    from pytorch_sound_amd import kernels as K
    F = 35
    c = _inputs(n, hop, None, F)
    plan = _plan(n, None)
    re, im, logit, gout = _dev(c['re']), _dev(c['im']), _dev(c['mask'][SIGMOID]), _dev(c['gout'])

    def run():
        leaves = [t.clone().requires_grad_(True) for t in (re, im, logit)]
        out = K.istft_reim(leaves[0], leaves[1], leaves[2], SIGMOID, n, hop, plan, 1e-9)
        out.backward(gout)
        m2 = logit.clone().requires_grad_(True)
        K.istft_reim(re, im, m2, SIGMOID, n, hop, plan, 0.0).backward(gout)
        return [out.detach()] + [t.grad for t in leaves] + [m2.grad]

    poison.assert_same_bits(run)


@pytest.mark.parametrize('n,hop', [(1024, 256), (400, 100)])
def test_forward_replays_from_a_captured_graph(n, hop):
    from pytorch_sound_amd import kernels as K
    F = 35
    plan = _plan(n, None)
    c = _inputs(n, hop, None, F)
    static = [_dev(c['re']).clone(), _dev(c['im']).clone(), _dev(c['mask'][SIGMOID]).clone()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            K.istft_reim(static[0], static[1], static[2], SIGMOID, n, hop, plan, 1e-9)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = K.istft_reim(static[0], static[1], static[2], SIGMOID, n, hop, plan, 1e-9)
    g = torch.Generator().manual_seed(99)
    for _ in range(3):
        fresh = [torch.randn(t.shape, generator=g) for t in static]
        for s, f in zip(static, fresh):
            s.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        eager = K.istft_reim(_dev(fresh[0]), _dev(fresh[1]), _dev(fresh[2]), SIGMOID, n, hop, plan, 1e-9)
        ref = _yardstick(fresh[0], fresh[1], fresh[2], SIGMOID, n, hop, c['window'])
        bound = _fwd_bound(n, ref)
        assert float((out.cpu().double() - ref).abs().max()) <= bound
        assert float((out - eager).abs().max()) <= bound


def _module(kind, n, hop):
    from pytorch_sound_amd.models.transforms import STFT, STFTTorchAudio
    return (STFT(n, hop) if kind == 'STFT' else STFTTorchAudio(n, hop)).to(DEV)


@pytest.mark.parametrize('kind,n,hop', [('STFT', 1024, 256), ('STFT', 1200, 300), ('STFTTorchAudio', 400, 100)])
def test_modules_round_trip_and_agree_with_the_polar_path(kind, n, hop):
    m = _module(kind, n, hop)
    T = 12 * hop
    x = torch.randn(2, T, generator=torch.Generator().manual_seed(n)) * 0.3
    xd = x.to(DEV)
    re, im = m.transform_complex(xd) if kind == 'STFT' else m(xd)
    rec = m.inverse_complex(re, im)
    assert rec.shape == (2, T)
    err = float((rec.cpu() - x).abs().max())
    print('%s(%d, %d): round trip %.3e' % (kind, n, hop, err))
    assert err <= 2e-5
    # the same spectrum through both inverses, each against float64
    window = torch.from_numpy(ofe.analysis_window(n))
    rec64 = _yardstick(re.cpu(), im.cpu(), None, NONE, n, hop, window)
    bound = _fwd_bound(n, rec64)
    assert float((rec.cpu().double() - rec64).abs().max()) <= bound
    from pytorch_sound_amd import kernels as K
    o = K.stft_forward(xd, n, hop, m._plan(xd.device), want_mag=True, want_phase=True, want_reim=True)
    polar = m.inverse(o['mag'], o['phase'])
    rect = m.inverse_complex(o['re'], o['im'])
    ref = _yardstick(o['re'].cpu(), o['im'].cpu(), None, NONE, n, hop, window)
    for name, got in (('inverse', polar), ('inverse_complex', rect)):
        e = float((got.cpu().double() - ref).abs().max())
        print('    %s against float64: %.3e (bound %.3e)' % (name, e, bound))
        assert e <= bound


def test_uncovered_size_raises_naming_the_covered_sizes():
    from pytorch_sound_amd import _lib
    from pytorch_sound_amd.models.transforms import STFT
    m = STFT(686, 98).to(DEV)
    x = torch.randn(1, 4000, device=DEV)
    with pytest.raises(_lib.PsndError, match='powers of two'):
        m.transform_complex(x)
    with pytest.raises(_lib.PsndError, match='powers of two'):
        m.inverse_complex(torch.randn(1, 344, 9, device=DEV), torch.randn(1, 344, 9, device=DEV))


@pytest.fixture
def collected():
    """the cases below build models and Trainers, which sit in reference cycles: the device memory they hold is released when the case ends,
    not by a garbage collection in the middle of a later test (tests/poison.py asserts that no block is freed while it fills the free ones)"""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _separator():
    from pytorch_sound_amd.models.separator import ConvSeparator
    from pytorch_sound_amd.models.transforms import STFT
    torch.manual_seed(5)
    return ConvSeparator(129, 64, 1).to(DEV), STFT(256, 64).to(DEV)


def test_separator_waveform_and_gradients(collected):
    from pytorch_sound_amd import kernels as K
    model, stft = _separator()
    n, hop = 256, 64
    x = (torch.randn(2, 4096, generator=torch.Generator().manual_seed(2)) * 0.5).to(DEV)
    gout = torch.randn(2, 4096, generator=torch.Generator().manual_seed(3))
    window = torch.from_numpy(ofe.analysis_window(n))
    kept = {}
    body = model.mask_logits

    def spy(mag):
        kept['logits'] = body(mag)
        kept['logits'].retain_grad()
        return kept['logits']

    model.mask_logits = spy
    with torch.autocast('cuda', dtype=torch.bfloat16):
        out = model.separate(x, stft)
        o = K.stft_forward(x, n, hop, stft._plan(x.device), want_mag=True, want_reim=True)
    logits = kept['logits']
    assert out.shape == (2, 4096) and out.dtype == torch.float32
    assert logits.shape == o['mag'].shape and logits.dtype == torch.float32
    leaf = logits.detach().cpu().double().requires_grad_(True)
    ref = _yardstick(o['re'].cpu(), o['im'].cpu(), leaf, SIGMOID, n, hop, window)
    err, bound = float((out.detach().cpu().double() - ref.detach()).abs().max()), _fwd_bound(n, ref.detach())
    print('separate against float64: %.3e (bound %.3e)' % (err, bound))
    assert err <= bound
    (out * gout.to(DEV)).sum().backward()
    (gref,) = torch.autograd.grad((ref * gout.double()).sum(), leaf)
    gerr, top = float((logits.grad.cpu().double() - gref).abs().max()), float(gref.abs().max())
    print('gradient at the logits: %.3e of max %.3e' % (gerr, top))
    assert gerr <= 1e-4 * top
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    with pytest.raises(RuntimeError, match='gradient'):
        model.separate(x.clone().requires_grad_(True), stft)
    del model.mask_logits


def _train(graph, steps=12):
    from pytorch_sound_amd.trainer import Trainer, LogType
    model, stft = _separator()
    g = torch.Generator().manual_seed(3)
    pool = [(torch.randn(4, 4096, generator=g) * 0.1, torch.randn(4, 4096, generator=g) * 0.1) for _ in range(steps)]

    class T(Trainer):
        def forward(self, noisy, clean, is_logging=False):
            with torch.autocast('cuda', dtype=torch.bfloat16):
                out = self.model.separate(noisy, stft)
            loss = (out - clean[:, :out.shape[1]]).abs().mean()
            return loss, {'loss': (loss, LogType.SCALAR)}

    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    tr = T(model, opt, pool, pool, max_step=10 ** 9, valid_max_step=1, save_interval=10 ** 9, log_interval=10 ** 9,
           save_dir=tempfile.mkdtemp(prefix='psnd_sep_'), seed=11)
    tr.graph_steps = graph
    model.train()
    for i in range(1, steps + 1):
        tr.step = i
        tr.train(i)
    torch.cuda.synchronize()
    tr._poll_nan_log(block=True)
    return [p.detach().float().clone() for p in model.parameters()], len(getattr(tr, '_graphs', {}))


def test_captured_training_steps_follow_eager_steps(collected):
    eager, n0 = _train(False)
    graph, n1 = _train(True)
    assert n0 == 0 and n1 == 1
    for a, b in zip(eager, graph):
        scale = float(a.abs().max()) + 1e-6
        assert float((a - b).abs().max()) <= 2e-2 * scale
    assert all(bool(np.isfinite(p.cpu().numpy()).all()) for p in graph)
