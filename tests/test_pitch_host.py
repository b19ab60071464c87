"""utils.pitch without a GPU: known answers through get_f0 on numpy arrays and CPU tensors (pure sines, a missing fundamental, other sample
rates, noise, silence, non-finite samples), the float64 host restatement against the yardstick tests/f0_ref.py, ragged batches, argument
errors, the alias import, and the host side of the C ABI (declared, exported, mirrored; every PSND_E_ARG case; psnd_yin_frames)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f0_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402


def _M():
    from pytorch_sound_amd.utils import pitch
    return pitch


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _interior(T, hop, span):
    """the frames whose whole span lies inside the signal"""
    H = span // 2
    return [i for i in range(T // hop + 1) if i * hop - H >= 0 and i * hop - H + span <= T]


def _sine(f, sr, T, phase=0.3):
    return np.sin(2.0 * np.pi * f * np.arange(T) / sr + phase).astype(np.float32)


def test_alias_is_the_same_module_and_sound_stays_as_it_was():
    import pytorch_sound.utils.pitch as a
    import pytorch_sound_amd.utils.pitch as b
    import pytorch_sound_amd.utils.sound as snd
    assert a is b and callable(a.get_f0) and callable(a.get_f0_with_confidence)
    assert not hasattr(snd, 'get_f0') and 'utils.pitch.get_f0' in snd.__doc__
    for word in ('YIN', 'WORLD', 'unpinned', 'not differentiable', 'unvoiced'):
        assert word.lower() in a.__doc__.lower(), word


def test_signature_is_the_references_and_more():
    import inspect
    M = _M()
    for fn in (M.get_f0, M.get_f0_with_confidence):
        p = list(inspect.signature(fn).parameters.values())
        assert [(q.name, q.default) for q in p[:3]] == [('wav', inspect.Parameter.empty), ('hop_length', inspect.Parameter.empty), ('sr', 22050)]
        assert [(q.name, q.default) for q in p[3:]] == [('f0_floor', 71.0), ('f0_ceil', 800.0), ('threshold', 0.1), ('frame_length', None),
                                                       ('lengths', None)]


def test_derived_values():
    K = _K()
    assert K.yin_lags(22050) == (27, 311, 622) == R.lags(22050)
    assert K.yin_lags(16000, 62.5) == (20, 256, 512)
    assert K.yin_lags(8000, 200.0) == (10, 40, 80)
    assert K.yin_lags(48000, 50.0) == (60, 960, 1920)
    assert K.yin_lags(1000, 71.0, 800.0) == (2, 15, 30)             # tau_min never under 2
    assert K.yin_lags(22050, frame_length=311) == (27, 311, 311)
    for T, hop in ((0, 256), (1, 256), (255, 256), (256, 256), (257, 256), (6000, 256)):
        assert K.yin_frames(T, hop) == T // hop + 1 == R.frames(T, hop)


def test_pure_sines():
    """forty frequencies from 75 to 790 Hz at 22.05 kHz, T = 6000, hop 256: every interior frame is voiced and within a relative 1e-3 of the
    true frequency.  The bound is 1.6 times the worst case of the float64 prototype of the definition, 6.3e-4: the bias of the parabola
    through three samples of d'.  Re-measured here: 6.25e-4 through get_f0 over all forty, and the same 6.25e-4 with tests/f0_ref.py on
    the four of them it is run on (the first, the last and two between); both are printed below."""
    M = _M()
    sr, T, hop = 22050, 6000, 256
    inner = _interior(T, hop, 933)
    assert len(inner) >= 15
    worst = worst_ref = 0.0
    for n, f in enumerate(np.linspace(75.0, 790.0, 40)):
        x = _sine(f, sr, T, 0.1 * n)
        got = M.get_f0(x, hop, sr)
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (T // hop + 1,)
        assert (got[inner] > 0).all(), f
        worst = max(worst, float(np.abs(got[inner] / f - 1.0).max()))
        if n % 13 == 0 or n == 39:
            ref = R.get_f0(x, hop, sr)[0]
            worst_ref = max(worst_ref, float(np.abs(ref[inner] / f - 1.0).max()))
            assert np.allclose(got, ref, rtol=1e-6, atol=0)
    print('pure sines: worst relative error %.3g (yardstick on four of them: %.3g)' % (worst, worst_ref))
    assert worst <= 1e-3


def test_missing_fundamental():
    M = _M()
    sr, T, hop = 22050, 6000, 256
    t = np.arange(T) / sr
    x = sum(np.sin(2 * np.pi * 150.0 * h * t + h) / h for h in (2, 3, 4, 5)).astype(np.float32)
    f0, ap = M.get_f0_with_confidence(x, hop, sr)
    inner = _interior(T, hop, 933)
    assert np.abs(f0[inner] / 150.0 - 1.0).max() < 1e-3 and (ap[inner] < 0.1).all()


@pytest.mark.parametrize('sr,hop', [(16000, 200), (44100, 512)])
def test_other_rates(sr, hop):
    M = _M()
    T = 5 * sr // 16
    x = _sine(123.4, sr, T)
    tau_min, tau_max, W = R.lags(sr)
    f0 = M.get_f0(torch.from_numpy(x), hop, sr)
    assert isinstance(f0, torch.Tensor) and f0.dtype == torch.float32 and f0.shape == (T // hop + 1,)
    inner = _interior(T, hop, W + tau_max)
    assert len(inner) >= 5
    err = np.abs(f0.numpy()[inner] / 123.4 - 1.0).max()
    print('123.4 Hz at %d Hz: worst relative error %.3g' % (sr, err))
    assert err <= 1e-4


def test_unvoiced_inputs():
    M = _M()
    sr, T, hop = 22050, 6000, 256
    noise = np.random.RandomState(3).randn(T).astype(np.float32)
    for x in (noise, np.zeros(T, np.float32)):
        f0, ap = M.get_f0_with_confidence(x, hop, sr)
        assert (f0 == 0).all() and (ap >= 0.1).all()
    assert (M.get_f0_with_confidence(np.zeros(T, np.float32), hop, sr)[1] == 1).all()        # d = 0 everywhere: d' = 1 by rule 2


@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
def test_a_non_finite_sample_zeroes_exactly_the_frames_that_hold_it(value):
    M = _M()
    sr, T, hop, at = 22050, 6000, 256, 3001
    x = _sine(200.0, sr, T)
    clean = M.get_f0_with_confidence(x, hop, sr)
    y = x.copy()
    y[at] = value
    f0, ap = M.get_f0_with_confidence(y, hop, sr)
    hit = R.spans_with(at, T, hop, 933)
    assert 3 <= len(hit) <= 4 and (clean[0][hit] > 0).all()
    rest = [i for i in range(T // hop + 1) if i not in hit]
    assert (f0[hit] == 0).all() and (ap[hit] == 1).all()
    assert np.array_equal(f0[rest], clean[0][rest]) and np.array_equal(ap[rest], clean[1][rest])
    ft = M.get_f0(torch.from_numpy(y), hop, sr)
    assert np.array_equal(ft.numpy(), f0)


def _vsv(sr=22050, T=9000):
    x = R.glide(sr, T)
    x[3500:5500] = 0.0
    return x


def test_voiced_silent_voiced_pattern_equals_the_yardstick():
    M = _M()
    x = _vsv()
    f0 = M.get_f0(x, 256)
    ref = R.get_f0(x, 256)
    assert np.array_equal(f0 > 0, ref[0] > 0)
    v = f0 > 0
    assert v[5:9].all() and not v[16:20].any() and v[26:31].all()


@pytest.mark.parametrize('cfg', range(4))
def test_host_restatement_against_the_yardstick(cfg):
    """lags equal on EVERY frame (float64 against float64: no frame is left out), f0 to 1e-12 relative"""
    K = _K()
    sr, hop, T, floor = R.CONFIGS[cfg]
    tau_min, tau_max, W = R.lags(sr, floor)
    for sigma in (0.0, 0.1):
        x = R.glide(sr, T, sigma, seed=cfg, quiet=(T // 2, 3 * T // 4) if sigma == 0 else None)
        f0, ap, lag = K.yin_f0_host(x, hop, float(sr), tau_min, tau_max, W, 0.1, chunk=7)
        rf, ra, rl, _ = R.track(x, hop, sr, tau_min, tau_max, W, 0.1)
        assert lag.dtype == np.int32 and np.array_equal(lag, rl)
        assert np.allclose(f0, rf, rtol=1e-12, atol=0) and np.allclose(ap, ra, rtol=1e-9, atol=0)
        assert (lag > 0).any() or cfg in (1, 3)         # 1: every span reaches over an end of the 700 samples; 3: five frames in all


def test_frame_length_variants_against_the_yardstick():
    K = _K()
    sr, hop, T = 8000, 64, 1500
    x = R.glide(sr, T, 0.05)
    for W in (113, 114, 151, 400):                      # W = tau_max, an odd H, an odd W, a long window
        tau_min, tau_max, _ = R.lags(sr, 71.0)
        assert tau_max == 113
        f0, ap, lag = K.yin_f0_host(x, hop, float(sr), tau_min, tau_max, W, 0.1)
        rf, ra, rl, _ = R.track(x, hop, sr, tau_min, tau_max, W, 0.1)
        assert np.array_equal(lag, rl) and np.allclose(f0, rf, rtol=1e-12, atol=0)


def test_lengths_equal_the_rows_cut_one_by_one():
    M, K = _M(), _K()
    sr, hop, T = 8000, 50, 1200
    lengths = [T, T - 1, hop, 0, 777]
    rows = np.stack([R.glide(sr, T, 0.02, seed=n) for n in range(5)])
    want = [M.get_f0_with_confidence(rows[n, :lengths[n]], hop, sr) for n in range(5)]
    dirty = rows.copy()
    for n in range(5):
        dirty[n, lengths[n]:] = np.float32(3.0e38) if n % 2 else np.nan
    F = T // hop + 1
    for batch in (rows, dirty, torch.from_numpy(dirty)):
        f0, ap = M.get_f0_with_confidence(batch, hop, sr, lengths=lengths)
        f0, ap = (np.asarray(f0), np.asarray(ap))
        assert f0.shape == ap.shape == (5, F) and f0.dtype == np.float32
        for n in range(5):
            k = lengths[n] // hop + 1
            assert np.array_equal(f0[n, :k], want[n][0]) and np.array_equal(ap[n, :k], want[n][1]), n
            assert (f0[n, k:] == 0).all() and (ap[n, k:] == 1).all()
    lag = K.yin_f0(torch.from_numpy(dirty), hop, sr, lengths=torch.tensor(lengths))[2]
    assert lag.dtype == torch.int32 and (lag[3] == 0).all() and (lag[0] > 0).any()
    three = M.get_f0(rows.reshape(5, 1, T), hop, sr)
    assert three.shape == (5, 1, F) and np.array_equal(three[:, 0], M.get_f0(rows, hop, sr))


def test_edges():
    M = _M()
    assert M.get_f0(np.zeros(0, np.float32), 256).tolist() == [0.0]          # T = 0: one frame
    assert M.get_f0(_sine(200.0, 22050, 100), 256).shape == (1,)            # T < hop
    assert M.get_f0(_sine(200.0, 22050, 700), 100).shape == (8,)            # T < span
    assert M.get_f0(np.zeros((0, 500), np.float32), 100).shape == (0, 6)
    assert M.get_f0(torch.zeros(3, 0), 100).shape == (3, 1)
    ints = (1000 * _sine(200.0, 22050, 3000)).astype(np.int16)
    assert np.array_equal(M.get_f0(ints, 256) > 0, M.get_f0(ints.astype(np.float32), 256) > 0)


def test_argument_errors():
    M, K = _M(), _K()
    x = _sine(200.0, 22050, 3000)
    for kw in (dict(hop_length=0), dict(hop_length=-3), dict(hop_length=2.5), dict(hop_length=True), dict(sr=0), dict(sr=-1.0),
               dict(sr=math.nan), dict(sr=math.inf), dict(f0_floor=0.0), dict(f0_floor=math.nan), dict(f0_ceil=-5.0),
               dict(f0_floor=900.0), dict(f0_ceil=50.0), dict(threshold=0.0), dict(threshold=-0.1), dict(threshold=math.nan),
               dict(frame_length=310), dict(frame_length=0), dict(frame_length=622.0)):
        a = dict(dict(hop_length=256, sr=22050), **kw)
        for wav in (x, torch.from_numpy(x)):
            with pytest.raises((ValueError, K.PsndError)):
                M.get_f0(wav, **a)
    with pytest.raises(K.PsndError):
        M.get_f0(torch.zeros(100, dtype=torch.int32), 10)
    with pytest.raises(K.PsndError):
        M.get_f0(torch.tensor(1.0), 10)
    with pytest.raises(K.PsndError):
        M.get_f0(np.zeros((2, 100), np.float32), 10, lengths=[100])
    with pytest.raises(K.PsndError):
        K.yin_f0(x, 256)                                                      # kernels takes tensors


# ---- the C ABI, host side -----------------------------------------------------------------------------------------------------------------
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
    for n in ('psnd_yin_frames', 'psnd_yin_max_span', 'psnd_yin_f0'):
        assert n + '(' in header and hasattr(h, n) and n in _lib.SIGNATURES, n
    res, args = _lib.SIGNATURES['psnd_yin_f0']
    assert res is ctypes.c_int and len(args) == 15
    P, I, F32, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    assert args == [P, I, I, P, I, I, I, I, F32, F64, P, P, P, I, P]
    assert 'psnd_yin_f0' in _lib.LAUNCHABLE and 'psnd_yin_frames' not in _lib.LAUNCHABLE
    assert lib.psnd_version() >= 147
    assert lib.psnd_yin_max_span() >= 960 + 1920


def test_frames_helper(lib):
    for hop in (1, 2, 256, 2000):
        for T in (0, 1, hop - 1, hop, hop + 1, 10 * hop + 3):
            assert lib.psnd_yin_frames(T, hop) == T // hop + 1, (T, hop)
    assert lib.psnd_yin_frames(100, 0) == 0 and lib.psnd_yin_frames(-1, 10) == 0


def test_bad_arguments_return_e_arg(lib):
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(x=p, N=1, T=1000, lengths=None, hop=100, W=80, tau_min=10, tau_max=40, threshold=0.1, sr=8000.0, f0=p, ap=p, lag=p, F=11,
              stream=None)
    top = lib.psnd_yin_max_span()

    def call(**kw):
        a = dict(ok, **kw)
        return lib.psnd_yin_f0(*[a[k] for k in ok])

    assert call(hop=0) == -1 and call(hop=-5) == -1
    assert b'yin' in lib.psnd_last_error()
    assert call(tau_min=1) == -1 and call(tau_min=0) == -1
    assert call(tau_max=9) == -1
    assert call(W=39) == -1
    for bad in (math.nan, 0.0, -0.1):
        assert call(threshold=bad) == -1 and call(sr=bad) == -1
    assert call(F=10) == -1 and call(F=0) == -1
    assert call(N=-1) == -1 and call(T=-1) == -1
    assert call(x=None) == -1 and call(f0=None) == -1 and call(ap=None) == -1 and call(lag=None) == -1
    assert call(W=top - 39) == -1 and call(W=top, tau_max=top) == -1 and call(W=2 ** 40) == -1      # a span beyond the LDS plan
    # nothing to do: nothing launched, no pointer looked at
    assert call(N=0) == 0 and call(N=0, x=None, f0=None, ap=None, lag=None) == 0
