"""The torch.stft-convention front ends on HIP tensors at FFT sizes that are no power of two (psnd_stft_mr_*: mixed-radix 2^a 3^b 5^c kernels):
STFTTorchAudio forward / transform / inverse with gradients, Audio2Mel, interface MelSpectrogram, LogMelSpectrogramTorchAudio and
multi_stft_loss, against the float64 oracle (oracle/features.py, oracle/sound.py).  At the parent of this change every case raised
PsndError when the plan was built.

Tolerances: (re, im, magnitude) 2e-5 of the largest bin, phase 2e-3 rad on bins above 1e-3 of the largest, waveform gradient through gmag or
(gre, gim) 5e-5 of its maximum (test_gpu_stft_modules.py::test_stft_any_filter_length_on_hip_tensors allows the same at these sizes), through
(magnitude, phase) together 2e-3 (test_stft_torchaudio_module); round trip 2e-5 max|x| + 2e-5; the inverse against istft_f64 2e-5 of its
maximum (the same fp32 transform error, spread by a window / envelope ratio of order one); log-mel 2e-4 absolute; multi_stft_loss as
test_gpu_sound.py (values 2e-5 relative, gradient 1e-2 of its maximum at eps = 1e-5 and 2e-4 at eps = 1e-2).  Every figure is printed
before it is asserted (`pytest -s`)."""
import functools

import numpy as np
import pytest
import torch

from conftest import seeded_wav
from oracle import features as ofe
from oracle import sound as osnd

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (n_fft, hop, win_length, T or None = 3 n + 37)
CASES = [(48, 12, None, None),          # 2^4 3
         (80, 20, None, None),          # 2^4 5
         (240, 60, 200, None),          # all three radices, short window, 13 frames (odd: the last one is paired with zeros)
         (400, 160, None, None),        # hop does not divide n
         (400, 77, None, None),         # odd hop
         (600, 600, None, None),        # no overlap
         (1200, 300, 1000, None),       # a common mid size, short window
         (4000, 1000, None, None),      # near the upper bound
         (3072, 768, None, None),       # a high power of two times 3
         (400, 160, None, 201),         # T = n / 2 + 1: the shortest signal a reflect pad allows (2 frames)
         (1200, 300, None, 2400)]       # 9 frames: odd, with T a multiple of the hop
IDS = ['%d-%d-%s-%s' % c for c in CASES]
N = 3


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(n, hop, win, T):
    """input and float64 references of one case, computed once and shared (read-only)"""
    T = T or 3 * n + 37
    wav = seeded_wav(n + hop, N, T)
    re, im = ofe.stft_reim_f64(wav, n, hop, win)
    mag = np.sqrt(re * re + im * im)
    r = np.random.RandomState(n + 7 * hop)
    g = [r.randn(*mag.shape) for _ in range(4)]          # gmag, gre, gim, gphase
    # The phase of a bin at the fp32 noise floor of the transform (|X| ~ 1e-6 of the largest bin occurs among 26 000 bins of noise) is
    # noise in any fp32 implementation, and d phase / d wav ~ 1 / |X| turns it into the whole gradient: torch's own fp32 stft -> atan2
    # -> autograd on the CPU sits 7.5e-3 (n = 4000) and 1.25e-2 (n = 1200, hop 300) of the maximum away from float64 on these very inputs
    # with a phase gradient on every bin.  The phase gradient therefore lives on the bins whose phase the forward check reads as well:
    # above 1e-3 of the largest.
    g[3] = g[3] * (mag > 1e-3 * mag.max())
    out = dict(T=T, wav=wav, re=re, im=im, mag=mag, g=g)
    for v in (wav, re, im, mag, *g):
        v.setflags(write=False)
    return out


def _module(n, hop, win):
    from pytorch_sound_amd.models.transforms import STFTTorchAudio
    return STFTTorchAudio(win or n, hop, win or n, n).to(DEV)


@pytest.mark.parametrize('n,hop,win,T', CASES, ids=IDS)
def test_forward_transform_backward(n, hop, win, T):
    from test_gpu_no_library_paths import forbid_library_ops
    c = _case(n, hop, win, T)
    m = _module(n, hop, win)
    wav, mag_ref = c['wav'], c['mag']
    sc = mag_ref.max()
    gmag, gre, gim, gph = [torch.from_numpy(a.astype(np.float32)).to(DEV) for a in c['g']]
    g64 = [_np(a).astype(np.float64) for a in (gmag, gre, gim, gph)]
    xs = [torch.from_numpy(wav).to(DEV).requires_grad_(True) for _ in range(3)]
    with forbid_library_ops():
        re, im = m(xs[0])
        (re * gre + im * gim).sum().backward()
        mag, ph = m.transform(xs[1])
        (mag * gmag).sum().backward()
        mag2, ph2 = m.transform(xs[2])
        (mag2 * gmag + ph2 * gph).sum().backward()
    assert re.shape == c['re'].shape == (N, n // 2 + 1, ofe.frame_count(c['T'], n, hop))
    e_re, e_im, e_mag = (np.abs(_np(a) - b).max() / sc for a, b in ((re, c['re']), (im, c['im']), (mag, mag_ref)))
    strong = mag_ref > 1e-3 * sc
    d = np.angle(np.exp(1j * (_np(ph).astype(np.float64) - np.arctan2(c['im'], c['re']))))
    e_ph = np.abs(d[strong]).max()
    want_reim = ofe.stft_reim_bwd_f64(g64[1], g64[2], c['T'], n, hop, win)
    want_mag = ofe.stft_mag_bwd_f64(g64[0], wav, n, hop, win)
    # (magnitude, phase) -> (re, im): d mag = (re d re + im d im) / mag, d phase = (re d im - im d re) / mag^2
    m2 = mag_ref ** 2
    pre = g64[0] * c['re'] / mag_ref - g64[3] * c['im'] / m2
    pim = g64[0] * c['im'] / mag_ref + g64[3] * c['re'] / m2
    want_polar = ofe.stft_reim_bwd_f64(pre, pim, c['T'], n, hop, win)
    e_g = [np.abs(_np(x.grad) - w).max() / np.abs(w).max() for x, w in zip(xs, (want_reim, want_mag, want_polar))]
    print('n=%d hop=%d win=%s T=%d: re %.2e im %.2e mag %.2e (of the largest bin) phase %.2e rad; gwav via (gre, gim) %.2e, gmag %.2e, '
          '(mag, phase) %.2e of its maximum' % (n, hop, win, c['T'], e_re, e_im, e_mag, e_ph, *e_g))
    assert max(e_re, e_im, e_mag) <= 2e-5
    assert e_ph <= 2e-3
    assert e_g[0] <= 5e-5 and e_g[1] <= 5e-5
    assert e_g[2] <= 2e-3
    assert torch.equal(mag, mag2) and torch.equal(ph, ph2)


def _istft_torch64(mag, phase, n, hop, window):
    """the overlap-add of psnd_istft restated on float64 torch tensors (CPU): differentiable in magnitude and phase"""
    Nb, K, F = mag.shape
    edge = torch.ones(K, 1, dtype=torch.float64)
    edge[0] = edge[-1] = 0.0                                     # the imaginary parts of DC and Nyquist do not reach the signal
    spec = torch.complex(mag * torch.cos(phase), mag * torch.sin(phase) * edge)
    fr = torch.fft.irfft(spec.transpose(1, 2), n=n, dim=-1) * window          # N, F, n
    L = (F - 1) * hop + n
    out = torch.zeros(Nb, L, dtype=torch.float64)
    env = torch.zeros(L, dtype=torch.float64)
    for f in range(F):
        out[:, f * hop:f * hop + n] += fr[:, f]
        env[f * hop:f * hop + n] += window * window
    env = torch.where(env > 0, env, torch.ones_like(env))       # zero only inside the trimmed edges
    return (out / env)[:, n // 2:L - n // 2]


@pytest.mark.parametrize('n,hop,win,T', [c for c in CASES if c[:2] != (600, 600)], ids=[i for i in IDS if not i.startswith('600-600')])
def test_inverse(n, hop, win, T):
    """(600, 600) is left out: a hann window without overlap has a vanishing envelope"""
    from test_gpu_no_library_paths import forbid_library_ops
    c = _case(n, hop, win, T)
    m = _module(n, hop, win)
    x = torch.from_numpy(c['wav']).to(DEV)
    F = c['mag'].shape[2]
    r = np.random.RandomState(3 * n + hop)
    rmag = np.abs(r.randn(N, n // 2 + 1, F)).astype(np.float32)
    rph = r.uniform(-np.pi, np.pi, rmag.shape).astype(np.float32)
    tm = torch.from_numpy(rmag).to(DEV).requires_grad_(True)
    tp = torch.from_numpy(rph).to(DEV).requires_grad_(True)
    with forbid_library_ops():
        rec = m.inverse(*m.transform(x))
        y = m.inverse(tm, tp)
        gy = torch.from_numpy(r.randn(*y.shape).astype(np.float32)).to(DEV)
        (y * gy).sum().backward()
    L = (F - 1) * hop
    assert rec.shape == (N, L) and y.shape == (N, L)
    e_rt = float((rec - x[:, :L]).abs().max())
    bound = 2e-5 * float(x.abs().max()) + 2e-5
    want = ofe.istft_f64(rmag, rph, n, hop, win, eps=0.0)
    e_inv = np.abs(_np(y) - want).max() / np.abs(want).max()
    cm = torch.from_numpy(rmag).double().requires_grad_(True)
    cp = torch.from_numpy(rph).double().requires_grad_(True)
    w64 = torch.from_numpy(ofe.analysis_window(n, win)).double()
    (_istft_torch64(cm, cp, n, hop, w64) * gy.cpu().double()).sum().backward()
    e_gm = float((tm.grad.cpu().double() - cm.grad).abs().max() / cm.grad.abs().max())
    e_gp = float((tp.grad.cpu().double() - cp.grad).abs().max() / cp.grad.abs().max())
    print('n=%d hop=%d win=%s T=%d: round trip %.2e (bound %.2e), inverse against istft_f64 %.2e of its maximum, gradient magnitude %.2e '
          'phase %.2e of its maximum' % (n, hop, win, c['T'], e_rt, bound, e_inv, e_gm, e_gp))
    assert e_rt <= bound
    assert e_inv <= 2e-5
    assert e_gm <= 5e-5 and e_gp <= 5e-5


# ---- mel front ends ----------------------------------------------------------------------------------------------------------------
def test_audio2mel_1200():
    from pytorch_sound_amd.models.transforms import Audio2Mel
    from test_gpu_no_library_paths import forbid_library_ops
    m = Audio2Mel(1200, 300, 1200, 24000, 80).to(DEV)
    wav = seeded_wav(1201, N, 3 * 1200 + 37, sr=24000)
    with forbid_library_ops():
        out = m(torch.from_numpy(wav).to(DEV).unsqueeze(1))
    want = ofe.hifigan_mel_f64(wav, _np(m.mel_basis).astype(np.float64), 1200, 300, 1200, log10=True)
    err = np.abs(_np(out) - want).max()
    print('Audio2Mel(1200, 300): %.2e' % err)
    assert out.shape == want.shape and err <= 2e-4
    x = torch.from_numpy(wav).to(DEV).unsqueeze(1).requires_grad_(True)        # the autograd route gives the same picture and a gradient
    o2 = m(x)
    o2.sum().backward()
    assert np.abs(_np(o2) - want).max() <= 2e-4 and bool(torch.isfinite(x.grad).all())


@pytest.mark.parametrize('is_center', [False, True])
def test_interface_melspectrogram_800(is_center):
    """mag_eps = 1e-9 inside the square root (interface/hifi_gan.py:46-63), both paddings"""
    from pytorch_sound_amd.interface.hifi_gan import MelSpectrogram
    m = MelSpectrogram(24000, 800, 800, 200, 80, 0., 8000.).to(DEV)
    wav = seeded_wav(801, N, 3 * 800 + 37, sr=24000)
    out = m(torch.from_numpy(wav).to(DEV), is_center=is_center)
    W = _np(m.mel_filter).astype(np.float64)
    if is_center:
        padded = np.pad(wav, ((0, 0), (m.pad_size, m.pad_size)), mode='reflect')
        mag = ofe.stft_mag_f64(padded, 800, 200, 800, ofe.CENTER, eps=1e-9)
        want = np.log(np.maximum(np.matmul(W, mag), 1e-5))
    else:
        want = ofe.hifigan_mel_f64(wav, W, 800, 200, 800, mag_eps=1e-9)
    err = np.abs(_np(out) - want).max()
    print('MelSpectrogram(800, 200, is_center=%s): %.2e' % (is_center, err))
    assert out.shape == want.shape and err <= 2e-4


def test_logmel_torchaudio_400():
    from pytorch_sound_amd.models.transforms import LogMelSpectrogramTorchAudio
    m = LogMelSpectrogramTorchAudio(16000, 40, 400, 400, 160, -80, 20).to(DEV)
    wav = seeded_wav(401, N, 3 * 400 + 37, sr=16000)
    x = torch.from_numpy(wav).to(DEV).requires_grad_(True)
    y = m(x)
    mag = ofe.stft_mag_f64(wav, 400, 160, 400)
    fb = _np(m.mel_filter).astype(np.float64)
    lin = np.matmul(fb, mag ** 2)
    lo, hi = np.log(10 ** -8.0), np.log(10 ** 2.0)
    want = np.clip(np.log(lin + 1e-6), lo, hi)
    err = np.abs(_np(y) - want).max()
    y.sum().backward()
    print('LogMelSpectrogramTorchAudio(400, 160): %.2e' % err)
    assert y.shape == want.shape and err <= 2e-4
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0


# ---- multi_stft_loss ---------------------------------------------------------------------------------------------------------------
MSL = [(1024, 600, 120), (1200, 1200, 300), (400, 400, 100)]


@pytest.mark.parametrize('eps,gtol', [(1e-5, 1e-2), (1e-2, 2e-4)])
@pytest.mark.parametrize('both', [False, True])
def test_multi_stft_loss_mixed_resolutions(eps, gtol, both):
    from pytorch_sound_amd.models.sound import build_stft_functions, multi_stft_loss
    from pytorch_sound_amd.models.transforms import centre_pad
    t = seeded_wav(604, 4, 6000)
    p = (0.8 * t + 0.05 * seeded_wav(704, 4, 6000)).astype(np.float32)
    pred = torch.from_numpy(p).to(DEV).requires_grad_(True)
    target = torch.from_numpy(t).to(DEV).requires_grad_(both)
    loss, sc, mag = multi_stft_loss(pred, target, MSL, eps)
    wins = [centre_pad(f.window.numpy().astype(np.float64), f.n_fft) for f in build_stft_functions(*MSL)]
    want = osnd.multi_stft_loss(p, t, MSL, eps, windows=wins)
    got = [float(loss), float(sc), float(mag)]
    print('multi_stft_loss eps=%g both=%s: got %r want %r' % (eps, both, got, want))
    assert np.allclose(got, want, rtol=2e-5), (got, want)
    if not both:
        loss.backward()
        gp = osnd.multi_stft_loss_grad(p, t, MSL, eps, windows=wins)
        e = np.abs(_np(pred.grad) - gp).max() / np.abs(gp).max()
        print('  prediction gradient %.2e of its maximum' % e)
        assert e <= gtol
        return
    (0.5 * loss + 2.0 * sc - 0.25 * mag).backward()
    L = len(MSL)
    gp, gt = np.zeros(p.shape), np.zeros(p.shape)
    for (n_fft, win, hop), w in zip(MSL, wins):
        pm = osnd.stft_mag_torchaudio_f64(p, n_fft, win, hop, w)
        tm = osnd.stft_mag_torchaudio_f64(t, n_fft, win, hop, w)
        a, b = osnd.stft_loss_terms_bwd(pm, tm, (0.5 + 2.0) / L, (0.5 - 0.25) / L, eps)
        gp += ofe.stft_mag_bwd_f64(a, p, n_fft, hop, framing=ofe.CENTER, window=w)
        gt += ofe.stft_mag_bwd_f64(b, t, n_fft, hop, framing=ofe.CENTER, window=w)
    e_p = np.abs(_np(pred.grad) - gp).max() / np.abs(gp).max()
    e_t = np.abs(_np(target.grad) - gt).max() / np.abs(gt).max()
    print('  gradients: prediction %.2e target %.2e of their maxima' % (e_p, e_t))
    assert e_p <= gtol and e_t <= gtol


def test_multi_stft_loss_refuses_uncovered_sizes():
    """the loss takes a narrower set than the plan (kernels.msl_covered): no multiple of 16 (600, and 1000 as test_gpu_sound.py pins),
    odd, a prime factor above 5 - PsndError before any launch, naming the covered sizes; the modules themselves run at 600 and 1000"""
    from pytorch_sound_amd import _lib
    from pytorch_sound_amd.models.sound import multi_stft_loss
    x = torch.from_numpy(seeded_wav(9, 2, 4096)).to(DEV)
    for res in [(600, 600, 150), (1000, 600, 120), (401, 401, 100), (686, 686, 98)]:
        with pytest.raises(_lib.PsndError, match='multiples of 16'):
            multi_stft_loss(x, x, [(1024, 600, 120), res])
    mag, _ = _module(1000, 250, None).transform(x)
    want = ofe.stft_mag_f64(_np(x), 1000, 250, None)
    assert np.abs(_np(mag) - want).max() <= 2e-5 * want.max()


# ---- reproducibility, capture, memory ----------------------------------------------------------------------------------------------
def _step(m, x, gmag, gph):
    xr = x.detach().requires_grad_(True)
    mag, ph = m.transform(xr)
    gw, = torch.autograd.grad([mag, ph], xr, [gmag, gph])
    rec = m.inverse(mag.detach(), ph.detach())
    return mag.detach(), ph.detach(), gw, rec


@pytest.mark.parametrize('n,hop', [(400, 160), (1200, 300)])
def test_bit_reproducible_and_capturable(n, hop):
    c = _case(n, hop, None, None)
    m = _module(n, hop, None)
    x = torch.from_numpy(c['wav']).to(DEV)
    gmag, gph = [torch.from_numpy(c['g'][i].astype(np.float32)).to(DEV) for i in (0, 3)]
    a = [t.clone() for t in _step(m, x, gmag, gph)]
    b = _step(m, x, gmag, gph)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(m, x, gmag, gph)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _step(m, x, gmag, gph)
    for _ in range(3):
        for o in out:
            o.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(a, out):
            assert torch.equal(u, v)


def test_every_output_element_is_written():
    """forward (all four outputs), both backward sources and the inverse on poisoned free memory (tests/poison.py): the outputs and the
    scratch come from torch.empty, so a gap in what the kernels write shows as a difference between the patterns.  9 frames: the last
    frame has no partner."""
    import poison
    from pytorch_sound_amd import kernels as K
    n, hop, T = 400, 160, 1300
    wav = torch.from_numpy(seeded_wav(5, N, T)).to(DEV)
    win = ofe.analysis_window(n)
    plan = K.stft_plan(n, win).to(DEV)
    F = ofe.frame_count(T, n, hop)
    assert F % 2 == 1
    r = np.random.RandomState(0)
    gs = [torch.from_numpy(r.randn(N, n // 2 + 1, F).astype(np.float32)).to(DEV) for _ in range(3)]

    def fn():
        o = K.stft_forward(wav, n, hop, plan, K.FRAMING_CENTER, 0.0, True, True, True)
        g1 = K.stft_backward(wav, n, hop, plan, K.FRAMING_CENTER, 0.0, gmag=gs[0])
        g2 = K.stft_backward(wav, n, hop, plan, K.FRAMING_CENTER, 0.0, gre=gs[1], gim=gs[2])
        g3 = K.stft_backward(wav, n, hop, plan, K.FRAMING_HIFIGAN, 1e-9, gmag=gs[0][:, :, :T // hop].contiguous(), gre=gs[1][:, :, :T // hop].contiguous(),
                             gim=gs[2][:, :, :T // hop].contiguous())
        y = K.istft_forward(o['mag'], o['phase'], n, hop, plan, 0.0)
        nopad = K.stft_forward(wav, n, hop, plan, K.FRAMING_NONE, 0.0, False, False, True)
        return [o['mag'], o['phase'], o['re'], o['im'], g1, g2, g3, y, nopad['re'], nopad['im']]

    poison.assert_same_bits(fn)


def test_rows_off_a_16_byte_boundary():
    from pytorch_sound_amd import kernels as K
    n, hop, T = 1200, 300, 3 * 1200 + 37
    c = _case(n, hop, None, None)
    plan = K.stft_plan(n, ofe.analysis_window(n)).to(DEV)
    aligned = torch.from_numpy(c['wav']).to(DEV)
    store = torch.empty(N * T + 1, dtype=torch.float32, device=DEV)
    shifted = store[1:].view(N, T)
    shifted.copy_(aligned)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    g = torch.from_numpy(c['g'][0].astype(np.float32)).to(DEV)
    oa = K.stft_forward(aligned, n, hop, plan, K.FRAMING_CENTER, 0.0, True, True, True)
    ob = K.stft_forward(shifted, n, hop, plan, K.FRAMING_CENTER, 0.0, True, True, True)
    for k in ('mag', 'phase', 're', 'im'):
        assert torch.equal(oa[k], ob[k])
    assert torch.equal(K.stft_backward(aligned, n, hop, plan, gmag=g), K.stft_backward(shifted, n, hop, plan, gmag=g))
    assert np.abs(_np(ob['mag']) - c['mag']).max() <= 2e-5 * c['mag'].max()
