"""Masked inverse STFT on (re, im) without a GPU: the host formulation (host.istft_complex) against float64 torch.istft and its autograd,
the argument checks of the three C entry points (psnd_istft_reim, psnd_istft_reim_mr, psnd_istft_reim_bwd) before they touch the device,
and ConvSeparator.separate on CPU tensors against the composed path."""
import ctypes
import os

import pytest
import torch

from oracle import features as ofe

NONE, LINEAR, SIGMOID = 0, 1, 2


@pytest.fixture(scope='module')
def L():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib


def _case(n_fft, hop, F, N=2, seed=0):
    g = torch.Generator().manual_seed(seed)
    K = n_fft // 2 + 1
    re, im = torch.randn(N, K, F, generator=g), torch.randn(N, K, F, generator=g)       # nonzero im at DC and Nyquist
    mask = torch.randn(N, K, F, generator=g) * 2
    mask[0, 3, 1] = 0.0
    return re, im, mask


def _yardstick(re, im, mask, kind, n_fft, hop, window):
    """float64 torch.istft(torch.complex(m re, m im), n_fft, hop, n_fft, window)"""
    re, im = re.double(), im.double()
    if kind != NONE:
        m = torch.sigmoid(mask.double()) if kind == SIGMOID else mask.double()
        re, im = m * re, m * im
    return torch.istft(torch.complex(re, im), n_fft, hop, n_fft, window.double())


@pytest.mark.parametrize('n_fft,hop,win', [(256, 64, None), (400, 100, None), (240, 60, 200)])
@pytest.mark.parametrize('kind', [NONE, LINEAR, SIGMOID])
@pytest.mark.parametrize('eps', [0.0, 1e-9])
def test_host_formulation_equals_float64_istft(n_fft, hop, win, kind, eps):
    from pytorch_sound_amd import host as H
    re, im, mask = _case(n_fft, hop, 9)
    window = torch.from_numpy(ofe.analysis_window(n_fft, win))
    if kind == SIGMOID:
        mask[0, 5, 2], mask[1, 7, 3] = 30.0, -30.0
    got = H.istft_complex(re, im, None if kind == NONE else mask, kind, n_fft, hop, window, eps)
    ref = _yardstick(re, im, mask, kind, n_fft, hop, window)
    assert got.shape == ref.shape == (2, 8 * hop)
    assert float((got.double() - ref).abs().max()) <= 1e-6 * float(ref.abs().max())


def test_host_formulation_without_a_mask_is_istft_of_magnitude_and_phase():
    from pytorch_sound_amd import host as H
    n_fft, hop = 256, 64
    re, im, _ = _case(n_fft, hop, 11, seed=1)
    window = torch.from_numpy(ofe.analysis_window(n_fft))
    a = H.istft_complex(re, im, None, None, n_fft, hop, window)
    b = H.istft(torch.sqrt(re * re + im * im), torch.atan2(im, re), n_fft, hop, window)
    assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


@pytest.mark.parametrize('kind', [LINEAR, SIGMOID])
def test_host_gradients_equal_float64_autograd(kind):
    from pytorch_sound_amd import host as H
    n_fft, hop = 256, 64
    re, im, mask = _case(n_fft, hop, 7, seed=2)
    window = torch.from_numpy(ofe.analysis_window(n_fft))
    gout = torch.randn(2, 6 * hop, generator=torch.Generator().manual_seed(5))
    leaves = [t.clone().requires_grad_(True) for t in (re, im, mask)]
    (H.istft_complex(leaves[0], leaves[1], leaves[2], kind, n_fft, hop, window, 0.0) * gout).sum().backward()
    ref = [t.double().clone().requires_grad_(True) for t in (re, im, mask)]
    (_yardstick(ref[0], ref[1], ref[2], kind, n_fft, hop, window) * gout.double()).sum().backward()
    for a, b in zip(leaves, ref):
        assert float((a.grad.double() - b.grad).abs().max()) <= 1e-5 * float(b.grad.abs().max())


def test_entry_points_validate_before_touching_the_device(L):
    lib = L.lib()
    assert lib.psnd_version() >= 143
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    r4 = lambda x: (x + 3) // 4 * 4          # noqa: E731

    # ---- psnd_istft_reim (power-of-two plans)
    inv = lambda **k: lib.psnd_istft_reim(*[k.get(a, d) for a, d in (            # noqa: E731
        ('re', p), ('im', p), ('mask', p), ('kind', LINEAR), ('N', 2), ('F', 9), ('n', 1024), ('hop', 256), ('plan', p), ('eps', 0.0),
        ('out', p), ('stream', None))])
    assert inv(re=None) == -1 and b'null' in lib.psnd_last_error()
    assert inv(im=None) == -1 and inv(plan=None) == -1 and inv(out=None) == -1
    assert inv(mask=None) == -1 and b'mask' in lib.psnd_last_error()             # LINEAR without a mask
    assert inv(mask=None, kind=SIGMOID) == -1
    assert inv(kind=NONE) == -1                                                  # a mask nobody asked for
    assert inv(kind=3) == -1 and inv(kind=-1) == -1
    assert inv(hop=0) == -1 and inv(F=-1) == -1
    assert inv(n=1001) == -4 and inv(n=1200) == -4                               # the mixed-radix sizes have their own entry point
    assert inv(N=0) == 0 and inv(F=1) == 0 and inv(F=0) == 0
    assert inv(N=0, mask=None, kind=NONE) == 0

    # ---- psnd_istft_reim_mr (mixed-radix plans)
    n, hop, F = 1200, 300, 9
    pb = lib.psnd_stft_mr_plan_bytes(n)
    ib = lib.psnd_istft_mr_scratch_bytes(2, F, n)
    mr = lambda **k: lib.psnd_istft_reim_mr(*[k.get(a, d) for a, d in (          # noqa: E731
        ('re', p), ('im', p), ('mask', p), ('kind', SIGMOID), ('N', 2), ('F', F), ('n', n), ('hop', hop), ('plan', p), ('pb', pb),
        ('eps', 0.0), ('scratch', p), ('sb', ib), ('out', p), ('stream', None))])
    assert mr(re=None) == -1 and mr(im=None) == -1 and mr(plan=None) == -1 and mr(out=None) == -1
    assert mr(mask=None) == -1 and mr(kind=NONE) == -1 and mr(kind=7) == -1
    assert mr(hop=0) == -1 and mr(F=-1) == -1
    assert mr(pb=pb - 4) == -1 and mr(pb=lib.psnd_stft_plan_bytes(1024)) == -1
    assert mr(scratch=None) == -1 and mr(sb=ib - 4) == -1 and b'scratch' in lib.psnd_last_error()
    assert mr(n=1001, pb=0) == -4 and mr(n=1024, pb=lib.psnd_stft_plan_bytes(1024)) == -4
    assert mr(N=0) == 0 and mr(F=1) == 0

    # ---- psnd_istft_reim_bwd (either plan kind)
    for n, hop, pb in ((1200, 300, lib.psnd_stft_mr_plan_bytes(1200)), (1024, 256, lib.psnd_stft_plan_bytes(1024)),
                       (128, 32, lib.psnd_stft_plan_bytes(128))):
        N, K = 3, n // 2 + 1
        sb = lib.psnd_istft_reim_bwd_scratch_bytes(N, F, n)
        assert sb == 4 * (r4(N * F * n) + 2 * r4(N * K * F)) > 0
        bwd = lambda **k: lib.psnd_istft_reim_bwd(*[k.get(a, d) for a, d in (    # noqa: E731
            ('g', p), ('re', p), ('im', p), ('mask', p), ('kind', SIGMOID), ('N', N), ('F', F), ('n', n), ('hop', hop), ('plan', p),
            ('pb', pb), ('eps', 0.0), ('scratch', p), ('sb', sb), ('g_re', p), ('g_im', p), ('g_mask', p), ('stream', None))])
        assert bwd(g=None) == -1 and bwd(plan=None) == -1
        assert bwd(re=None) == -1 and bwd(im=None) == -1                         # g_mask is formed from re and im
        assert bwd(g_re=None) == -1 and bwd(g_im=None) == -1                     # together or not at all
        assert bwd(g_re=None, g_im=None, g_mask=None) == -1                      # nothing requested
        assert bwd(mask=None) == -1 and bwd(kind=NONE) == -1 and bwd(kind=3) == -1
        assert bwd(mask=None, kind=NONE) == -1                                   # g_mask without a mask
        assert bwd(hop=0) == -1 and bwd(F=-1) == -1
        assert bwd(pb=pb - 4) == -1 and b'plan' in lib.psnd_last_error()
        assert bwd(scratch=None) == -1 and bwd(sb=sb - 4) == -1 and b'scratch' in lib.psnd_last_error()
        assert bwd(N=0) == 0 and bwd(F=1) == 0
        assert bwd(N=0, g_re=None, g_im=None) == 0                               # the mask-only call
        assert bwd(N=0, mask=None, kind=NONE, g_mask=None) == 0                  # no mask: (g_re, g_im) alone
    assert lib.psnd_istft_reim_bwd_scratch_bytes(3, F, 1001) == 0
    assert lib.psnd_istft_reim_bwd_scratch_bytes(0, F, 1024) == 0 and lib.psnd_istft_reim_bwd_scratch_bytes(3, 1, 1024) == 0
    assert lib.psnd_istft_reim_bwd(p, p, p, p, SIGMOID, 3, F, 1001, 250, p, 0, 0.0, p, 1 << 20, p, p, p, None) == -4


def test_python_front_end_rejects_host_tensors_and_bad_masks(L):
    from pytorch_sound_amd import kernels as K
    assert (K.MASK_NONE, K.MASK_LINEAR, K.MASK_SIGMOID) == (0, 1, 2)
    re, im, mask = _case(256, 64, 5)
    plan = K.stft_plan(256, ofe.analysis_window(256))
    with pytest.raises(L.PsndError):
        K.istft_reim(re, im, mask, K.MASK_SIGMOID, 256, 64, plan)                # no CPU fallback behind the kernels module


@pytest.mark.parametrize('kind', ['STFT', 'STFTTorchAudio'])
def test_module_methods_on_cpu_tensors(kind):
    from pytorch_sound_amd.models.transforms import STFT, STFTTorchAudio
    m = STFT(400, 100) if kind == 'STFT' else STFTTorchAudio(400, 100)
    x = torch.randn(2, 2000, generator=torch.Generator().manual_seed(3)) * 0.3
    re, im = m.transform_complex(x) if kind == 'STFT' else m(x)
    rec = m.inverse_complex(re, im)
    assert rec.shape == (2, 2000) and float((rec - x).abs().max()) <= 2e-5
    mag, phase = m.transform(x)
    mask = torch.rand(re.shape, generator=torch.Generator().manual_seed(4))
    a, b = m.inverse_complex(re, im, mask), m.inverse(mask * mag, phase)
    assert float((a - b).abs().max()) <= 1e-5


def test_separate_on_cpu_equals_the_composed_path():
    from pytorch_sound_amd.models.separator import ConvSeparator
    from pytorch_sound_amd.models.transforms import STFT, STFTTorchAudio
    torch.manual_seed(0)
    model = ConvSeparator(129, 16, 1).eval()
    x = torch.randn(2, 2048, generator=torch.Generator().manual_seed(1)) * 0.5    # unit-scale audio
    for stft in (STFT(256, 64), STFTTorchAudio(256, 64)):
        with torch.no_grad():
            mag, phase = stft.transform(x)
            want = stft.inverse(model(mag), phase)
            got = model.separate(x, stft)
            logits = model.mask_logits(mag)
            est = model(mag)
        assert got.shape == want.shape == (2, 2048)
        assert float((got - want).abs().max()) <= 1e-5
        assert logits.shape == mag.shape and logits.dtype == torch.float32
        assert float((torch.sigmoid(logits) * mag - est).abs().max()) <= 1e-6
    with pytest.raises(RuntimeError, match='gradient'):
        model.separate(x.clone().requires_grad_(True), STFT(256, 64))
    out = model.separate(x, STFT(256, 64))                                        # differentiable in the parameters
    out.abs().mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
