"""Griffin-Lim without a GPU: kernels.griffinlim_step_host / griffinlim_start_host against the yardstick tests/gl_ref.py, the whole loop on
CPU tensors (a fixed point at the true phase, a convergence measure that does not rise, n_iter = 0, length, dtypes, the numpy round trip,
utils.sound.griffinlim and models.sound.GriffinLim), argument errors of the Python entries and - through ctypes - of psnd_griffinlim_start
and psnd_griffinlim_step."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _U():
    from pytorch_sound_amd.utils import sound
    return sound


def _stft(n_fft, hop):
    from pytorch_sound_amd.models.transforms import STFT
    return STFT(n_fft, hop)


def _spectrum(x, stft):
    """(mag, phase) float64 tensors (N, K, F) of float32 clips (N, T) through the host transform in float64"""
    re, im = stft.transform_complex(torch.from_numpy(np.asarray(x, np.float64)))
    return torch.hypot(re, im), torch.atan2(im, re)


# ---- the host restatement against the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', (0.0, 0.99 / 1.99))
@pytest.mark.parametrize('with_p', (False, True))
def test_host_step_is_the_yardstick(alpha, with_p):
    K = _K()
    S, cr, ci, pr, pi = R.planes(3, 5, 41, seed=1)
    S[1, 2, 5:9] = 0.0
    cr[2, 0, 3], ci[2, 0, 3] = 0.0, 0.0                  # t = 0 without P
    p = (pr, pi) if with_p else (None, None)
    xr, xi, sums = K.griffinlim_step_host(S, cr, ci, p[0], p[1], alpha)
    want = R.step(S, cr, ci, p[0], p[1], alpha)
    err = R.rel_err((xr, xi), want)
    print('alpha %g, P %s: host step against the yardstick %.3g' % (alpha, with_p, err))
    assert xr.dtype == np.float64 and xr.shape == (3, 5, 41) and err <= 1e-14
    assert (xr[1, 2, 5:9] == 0).all() and (xi[1, 2, 5:9] == 0).all()
    if not with_p:
        assert xr[2, 0, 3] == 0 and xi[2, 0, 3] == 0
    part = R.partial(S, cr, ci, 5 * 41)
    assert sums.shape == (3, 2) and R.rel_err(sums, part[:, 0]) <= 1e-13
    part = R.partial(S, cr, ci, 64)                     # any chunking adds up to the item's sums
    assert R.rel_err(sums, part.sum(axis=1)) <= 1e-13


def test_host_step_ragged_and_start():
    K = _K()
    S, cr, ci, pr, pi = R.planes(6, 3, 24, seed=2)
    fr = [0, 1, 24, 33, -2, 7]
    for n, fn in enumerate(fr):
        fn = min(max(fn, 0), 24)
        for a in (S, cr, ci, pr, pi):
            a[n, :, fn:] = np.nan                       # behind an item's frames nothing is read
    xr, xi, sums = K.griffinlim_step_host(S, cr, ci, pr, pi, 0.4, frames=fr)
    want = R.step(S, cr, ci, pr, pi, 0.4, frames=fr)
    assert np.isfinite(xr).all() and np.isfinite(sums).all() and R.rel_err((xr, xi), want) <= 1e-14
    assert (xr[0] == 0).all() and (xr[1, :, 1:] == 0).all() and (xi[5, :, 7:] == 0).all() and np.abs(xr[2]).max() > 0.1
    assert R.rel_err(sums, R.partial(S, cr, ci, 3 * 24, fr)[:, 0]) <= 1e-13 and (sums[0] == 0).all() and (sums[4] == 0).all()
    x0 = K.griffinlim_start_host(S, pr, fr)
    assert np.isfinite(x0[0]).all() and R.rel_err(x0, R.start(S, pr, fr)) <= 1e-14
    x0 = K.griffinlim_start_host(S, None, fr)
    assert np.array_equal(x0[0], np.where(np.isnan(S), 0.0, S)) and (x0[1] == 0).all()
    # tensors: the CPU road of the device functions, cast back to the input's dtype
    t = [torch.from_numpy(a) for a in (S, cr, ci, pr, pi)]
    got = K.griffinlim_step(*t, alpha=0.4, frames=fr, partial=True)
    assert got[0].dtype == torch.float32 and np.array_equal(got[0].numpy(), xr.astype(np.float32)) and got[2].shape == (6, 1, 2)
    assert np.array_equal(got[2].numpy()[:, 0], sums)
    got = K.griffinlim_start(t[0], t[3], frames=torch.tensor(fr, dtype=torch.int32))
    assert np.array_equal(got[1].numpy(), K.griffinlim_start_host(S, pr, fr)[1].astype(np.float32))


# ---- the whole loop on CPU tensors ----------------------------------------------------------------------------------------------------------
def test_fixed_point_at_the_true_phase():
    """momentum 0, 2 iterations, STFT(256, 64), T = 8192: the loop started at the true phase returns the waveform, edges included"""
    K = _K()
    stft = _stft(256, 64)
    x = np.stack([R.clip(8192, 1), R.clip(8192, 2)])
    mag, phase = _spectrum(x, stft)
    y = K.griffinlim(mag, stft, n_iter=2, momentum=0.0, init_phase=phase)
    err = float((y - torch.from_numpy(x).double()).abs().max())
    print('fixed point, float64: %.3g' % err)
    assert y.dtype == torch.float64 and y.shape == (2, 8192) and not y.requires_grad and err <= 1e-8
    y0 = K.griffinlim(mag, stft, n_iter=0, init_phase=phase)                    # n_iter = 0: the inverse of X0
    assert float((y0 - stft.inverse_complex(mag * torch.cos(phase), mag * torch.sin(phase))).abs().max()) <= 1e-12


@pytest.mark.parametrize('n_fft, hop, T', [(256, 64, 8192), (400, 100, 8000)])
def test_convergence_does_not_rise_and_the_loop_is_the_yardsticks(n_fft, hop, T):
    K = _K()
    stft = _stft(n_fft, hop)
    x = np.stack([R.clip(T, 3), R.clip(T, 4)])
    mag, _ = _spectrum(x, stft)
    phi = torch.from_numpy(np.random.RandomState(5).uniform(0, 2 * np.pi, tuple(mag.shape)))
    y, conv = K.griffinlim(mag, stft, n_iter=16, momentum=0.0, init_phase=phi, return_convergence=True)
    print('conv, momentum 0:', conv[:, 0].numpy().round(4))
    assert conv.shape == (16, 2) and conv.dtype == torch.float64
    assert bool((conv[1:] <= conv[:-1]).all()) and float(conv[-1].max()) < 0.6 * float(conv[0].min())
    want_y, want_c = R.loop(mag.numpy(), stft, 16, 0.0, phi.numpy())
    assert R.rel_err(y.numpy(), want_y) <= 1e-10 and R.rel_err(conv.numpy(), want_c) <= 1e-10
    y2, conv2 = K.griffinlim(mag, stft, n_iter=16, momentum=0.99, init_phase=phi, return_convergence=True)
    print('conv, momentum 0.99:', conv2[:, 0].numpy().round(4))
    assert float(conv2[-1].max()) < float(conv[-1].min())                        # the fast variant is faster on this clip
    want_y, want_c = R.loop(mag.numpy(), stft, 16, 0.99, phi.numpy())
    assert R.rel_err(y2.numpy(), want_y) <= 1e-9 and R.rel_err(conv2.numpy(), want_c) <= 1e-9
    # the float32 variant of the yardstick stays close: what the GPU tests' bound is made of
    var_y, _ = R.loop(mag.float().numpy(), stft, 8, 0.99, phi.float().numpy(), dtype=np.float32)
    ref_y, _ = R.loop(mag.float().numpy(), stft, 8, 0.99, phi.float().numpy())
    print('float32 variant after 8 iterations: %.3g' % R.rel_err(var_y, ref_y))
    assert R.rel_err(var_y, ref_y) < 1e-3


def test_lengths_dtypes_shapes_and_the_numpy_round_trip():
    K, U = _K(), _U()
    from pytorch_sound_amd.models.sound import GriffinLim
    stft = _stft(256, 64)
    x = R.clip(4096, 6)[None]
    mag, _ = _spectrum(x, stft)
    F = mag.shape[-1]
    m32 = mag.float()
    y = K.griffinlim(m32, stft, n_iter=3, rand_init=False)
    assert y.dtype == torch.float32 and y.shape == (1, (F - 1) * 64)
    assert torch.equal(y, K.griffinlim(mag.float().double(), stft, n_iter=3, rand_init=False).float())     # float64 inside, cast back
    assert torch.equal(K.griffinlim(m32, stft, n_iter=3, rand_init=False, length=1000), y[:, :1000])
    long = K.griffinlim(m32, stft, n_iter=3, rand_init=False, length=5000)
    assert long.shape == (1, 5000) and torch.equal(long[:, :4096], y) and bool((long[:, 4096:] == 0).all())
    assert torch.equal(K.griffinlim(m32[0], stft, n_iter=3, rand_init=False), y[0])                        # (K, F): one item
    assert torch.equal(K.griffinlim(m32[None], stft, n_iter=3, rand_init=False), y[None])                  # a leading extra axis
    assert K.griffinlim(m32.half(), stft, n_iter=1, rand_init=False).dtype == torch.float16
    # the random start: reproducible through a generator, different without one
    g = lambda: torch.Generator().manual_seed(11)                                                          # noqa: E731
    a, b = K.griffinlim(m32, stft, n_iter=2, generator=g()), K.griffinlim(m32, stft, n_iter=2, generator=g())
    assert torch.equal(a, b) and not torch.equal(a, K.griffinlim(m32, stft, n_iter=2))
    phi = 2.0 * math.pi * torch.rand(m32.shape, generator=g())
    assert torch.equal(a, K.griffinlim(m32, stft, n_iter=2, init_phase=phi))                               # init_phase overrides rand_init
    # utils.sound: numpy in, float32 numpy out; n_fft and hop_length from the shape
    u = U.griffinlim(m32.numpy(), n_iter=3, rand_init=False)
    assert isinstance(u, np.ndarray) and u.dtype == np.float32 and np.array_equal(u, y.numpy())
    assert np.array_equal(U.griffinlim(mag.numpy(), 3, 256, 64, 0.99, None, None, False), y.numpy())      # float64 numpy in: float32 out
    assert torch.equal(U.griffinlim(m32, 3, rand_init=False), y) and U.griffinlim(mag, 1, rand_init=False).dtype == torch.float64
    assert np.array_equal(U.griffinlim(m32.numpy(), 2, init_phase=phi.numpy()), a.numpy())
    assert U.griffinlim(m32.numpy(), 1, hop_length=32, rand_init=False).shape == (1, (F - 1) * 32)
    # the module
    m = GriffinLim(256, 64, n_iter=3, rand_init=False)
    assert torch.equal(m(m32), y) and torch.equal(m(m32[0]), y[0]) and not list(m.parameters()) and torch.equal(m(m32, 1000), y[:, :1000])
    p2 = GriffinLim(256, 64, n_iter=3, power=2.0, rand_init=False)
    assert torch.equal(p2(m32 ** 2), K.griffinlim((m32 ** 2) ** 0.5, stft, n_iter=3, rand_init=False))
    assert 'n_iter=3' in repr(m) and 'power=2.0' in repr(p2)
    with pytest.raises(RuntimeError):
        m(m32[None])
    import pytorch_sound.utils.sound as a_u
    import pytorch_sound.models.sound as a_m
    assert callable(a_u.griffinlim) and hasattr(a_m, 'GriffinLim')


def test_a_tone_comes_back_on_its_bin():
    """16 iterations from the magnitude alone, zero first phase: the peak of the result sits on the tone's bin"""
    K = _K()
    stft = _stft(256, 64)
    T, k = 8192, 20
    x = (0.5 * np.sin(2 * np.pi * k / 256.0 * np.arange(T) + 0.4)).astype(np.float32)[None]
    mag, _ = _spectrum(x, stft)
    y = K.griffinlim(mag.float(), stft, n_iter=16, rand_init=False)[0].double().numpy()
    inner = y[256:-256]
    peak = int(np.abs(np.fft.rfft(inner * np.hanning(inner.size))).argmax())
    assert peak == round(k / 256.0 * inner.size), (peak, k / 256.0 * inner.size)
    assert np.abs(inner).max() > 0.25


def test_argument_errors_of_the_python_entries():
    K, U = _K(), _U()
    from pytorch_sound_amd.models.sound import GriffinLim
    stft = _stft(256, 64)
    mag = torch.ones(1, 129, 20)
    for bad in (-1, 1.5, None, True, '3'):
        with pytest.raises(ValueError):
            K.griffinlim(mag, stft, n_iter=bad)
    for bad in (-0.1, 1.0, 2.0, math.nan, 'x', None, True):
        with pytest.raises(ValueError):
            K.griffinlim(mag, stft, momentum=bad)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError):
            K.griffinlim(mag, stft, length=bad)
    with pytest.raises(K.PsndError):
        K.griffinlim(mag.numpy(), stft)                                         # kernels takes tensors
    with pytest.raises(K.PsndError, match='bins'):
        K.griffinlim(torch.ones(1, 100, 20), stft)
    with pytest.raises(K.PsndError):
        K.griffinlim(torch.ones(129), stft)
    with pytest.raises(K.PsndError):
        K.griffinlim(mag.int(), stft)
    with pytest.raises(K.PsndError):
        K.griffinlim(mag, stft, init_phase=torch.zeros(1, 129, 21))
    with pytest.raises(K.PsndError):
        K.griffinlim(mag, stft, init_phase=torch.zeros(1, 129, 20, dtype=torch.float64))
    with pytest.raises(K.PsndError, match='reflect'):
        K.griffinlim(torch.ones(1, 129, 3), stft)                               # 128 samples: not more than n_fft / 2
    with pytest.raises(K.PsndError):
        K.griffinlim(mag, stft, frames=[20, 20])
    with pytest.raises(K.PsndError):
        K.griffinlim(mag, stft, frames=[20.0])
    with pytest.raises(K.PsndError):
        K.griffinlim_step(mag, mag, mag, mag, None)                             # one of pre / pim
    with pytest.raises(K.PsndError):
        K.griffinlim_step(mag, mag, torch.ones(1, 129, 21))
    with pytest.raises(K.PsndError):
        K.griffinlim_step(mag, mag, mag.double())
    with pytest.raises(K.PsndError):
        K.griffinlim_step(mag, mag, mag, out=(mag.clone(), mag.clone()))        # out is for HIP tensors
    with pytest.raises(ValueError):
        K.griffinlim_step_host(mag.numpy(), mag.numpy(), np.ones((1, 129, 21)))
    with pytest.raises(ValueError):
        K.griffinlim_step_host(mag.numpy(), mag.numpy(), mag.numpy(), mag.numpy(), None)
    with pytest.raises(K.PsndError):
        U.griffinlim(np.ones(129, np.float32))
    with pytest.raises(ValueError):
        GriffinLim(power=0.0)
    with pytest.raises(ValueError):
        GriffinLim(momentum=1.0)
    assert 'gradients through the loop are out of scope' in K.griffinlim.__doc__ and 'off the iterated path' in K.griffinlim.__doc__.lower()
    for word in ('griffinlim', 'torchaudio', 'librosa', 'no parity to pin', 'perraudin'):
        assert word in ' '.join(U.__doc__.lower().split()), word


# ---- the C ABI, host side -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.lib()


def test_entries_are_declared_exported_and_mirrored(lib):
    from pytorch_sound_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'psnd.h')).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for n in ('psnd_gl_chunk', 'psnd_gl_chunks', 'psnd_griffinlim_start', 'psnd_griffinlim_step'):
        assert n + '(' in header and hasattr(h, n) and n in _lib.SIGNATURES, n
    P, I, F32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert _lib.SIGNATURES['psnd_griffinlim_start'] == (ctypes.c_int, [P, P, I, I, I, P, P, P, P])
    assert _lib.SIGNATURES['psnd_griffinlim_step'] == (ctypes.c_int, [P, P, P, P, P, I, I, I, P, F32, F32, P, P, P, P])
    assert _lib.SIGNATURES['psnd_gl_chunks'] == (ctypes.c_int64, [I, I])
    assert {'psnd_griffinlim_start', 'psnd_griffinlim_step'} <= set(_lib.LAUNCHABLE) and 'psnd_gl_chunk' not in _lib.LAUNCHABLE
    assert lib.psnd_version() >= 149
    C = lib.psnd_gl_chunk()
    assert C == _K().gl_chunk() and C > 0 and C % 256 == 0
    for K_, F_, want in ((1, 1, 1), (1, C, 1), (1, C + 1, 2), (3, C, 3), (513, 2584, -(-513 * 2584 // C)), (0, 5, 0), (5, 0, 0), (-1, 5, 0)):
        assert lib.psnd_gl_chunks(K_, F_) == want == _K().gl_chunks(K_, F_), (K_, F_)
    # enough workgroups on the flagship shape to cover 256 compute units several times over, also for one clip
    assert 32 * lib.psnd_gl_chunks(513, 2584) >= 16 * 256 and lib.psnd_gl_chunks(513, 2584) >= 2 * 256


def test_bad_arguments_return_e_arg(lib):
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(mag=p, cre=p, cim=p, pre=p, pim=p, N=1, K=2, F=100, frames=None, alpha=0.5, eps=1e-16, xre=p, xim=p, partial=None, stream=None)

    def step(**kw):
        a = dict(ok, **kw)
        return lib.psnd_griffinlim_step(*[a[k] for k in ok])

    ok0 = dict(mag=p, phase=p, N=1, K=2, F=100, frames=None, xre=p, xim=p, stream=None)

    def start(**kw):
        a = dict(ok0, **kw)
        return lib.psnd_griffinlim_start(*[a[k] for k in ok0])

    for call in (step, start):
        assert call(N=-1) == -1 and call(K=-1) == -1 and call(F=-1) == -1
        assert b'griffinlim' in lib.psnd_last_error()
        assert call(mag=None) == -1 and call(xre=None) == -1 and call(xim=None) == -1
        assert b'null' in lib.psnd_last_error()
        assert call(K=2 ** 20, F=2 ** 11) == -2 and call(K=2 ** 40, F=2 ** 40) == -2                # 2^31 elements per item and beyond
        assert call(N=2 ** 31, K=1, F=1) == -2                                                     # more than 2^31 - 1 workgroups
        # nothing to do: nothing launched, no pointer looked at
        none = dict(mag=None, xre=None, xim=None)
        assert call(N=0, **none) == 0 and call(K=0, **none) == 0 and call(F=0, **none) == 0
    assert step(cre=None) == -1 and step(cim=None) == -1
    assert step(pre=None) == -1 and step(pim=None) == -1                                           # exactly one of the pair
    assert b'pre and pim' in lib.psnd_last_error()
