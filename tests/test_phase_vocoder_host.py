"""The phase vocoder without a GPU: kernels.phase_vocoder_host against the loop yardstick tests/pv_ref.py, the yardstick against the textbook
wording (expected advance, wrap, cumsum), known answers (rate = 1, rotating rows in closed form), pv_frames against counting, the pinned
pitch_ratio table, argument errors of the Python entries and - through ctypes - of psnd_phase_vocoder, and utils.sound.time_stretch /
pitch_shift / models.sound.TimeStretch / PitchShift on numpy arrays and CPU tensors (lengths, the three-call composition, peak bins)."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pv_ref as R  # noqa: E402
from conftest import ROOT, seeded_wav  # noqa: E402

RATES = (1.0, 0.5, 2.0, 0.8, 1.25, 1.0 / 3.0, 3.7)


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _U():
    from pytorch_sound_amd.utils import sound
    return sound


def _stft_of(wav, n_fft, hop):
    """(re, im) float64 (K, F) of one clip through the host STFT of the project"""
    from pytorch_sound_amd.models.transforms import STFT
    re, im = STFT(n_fft, hop).transform_complex(torch.from_numpy(np.asarray(wav, np.float32))[None])
    return re[0].double().numpy(), im[0].double().numpy()


# ---- the host restatement against the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rate', RATES + (0.03, 40.0))
def test_host_function_is_the_yardstick(rate):
    K = _K()
    re, im = R.seeded_spectrum(2, 3, 97, seed=1)
    re[1, 20:31] = im[1, 20:31] = 0.0                   # arg 0 = 0
    re[1, 25], im[1, 26] = -0.0, -0.0
    re[4] = im[4] = 0.0
    got = K.phase_vocoder_host(re.reshape(2, 3, 97), im.reshape(2, 3, 97), rate)
    want = R.pv(re, im, rate)
    assert got[0].shape == (2, 3, K.pv_frames(97, rate)) and got[0].dtype == np.float64
    err = R.rel_err((got[0].reshape(6, -1), got[1].reshape(6, -1)), want)
    print('rate %g: host function against the yardstick %.3g' % (rate, err))
    assert err <= 1e-12
    assert (got[0][1, 1] == 0).all() and (got[1][1, 1] == 0).all()


def test_host_function_ragged_and_non_finite():
    K = _K()
    re, im = R.seeded_spectrum(5, 2, 40, seed=2)
    fr = [0, 1, 40, 55, -3]
    re[5, 17], im[4, 30] = np.nan, np.inf               # item 2: rows 4 and 5
    re[3, 20] = np.nan                                  # item 1 has one frame: behind its length, never read
    got = K.phase_vocoder_host(re.reshape(5, 2, 40), im.reshape(5, 2, 40), 0.8, np.array(fr).reshape(5, 1))
    want = R.pv(re, im, 0.8, np.repeat(fr, 2))
    assert R.rel_err((got[0].reshape(10, -1), got[1].reshape(10, -1)), want) <= 1e-12
    first = {5: min(j for j in range(50) if int(j * 0.8) + 1 >= 17), 4: min(j for j in range(50) if int(j * 0.8) + 1 >= 30)}
    for row, j in first.items():
        y = got[0].reshape(10, -1)[row]
        assert np.isnan(y[j:]).all() and np.isfinite(y[:j]).all(), row
    assert np.isfinite(got[0][1]).all() and (got[0][1][:, 2:] == 0).all() and (got[0][0] == 0).all() and (got[0][4] == 0).all()
    t = K.phase_vocoder(torch.from_numpy(re).reshape(5, 2, 40), torch.from_numpy(im).reshape(5, 2, 40), 0.8, frames=fr)
    assert t[0].dtype == torch.float32 and np.array_equal(t[0].numpy(), got[0].astype(np.float32), equal_nan=True)


# ---- the yardstick against the textbook -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T, rate', [(12800, 0.8), (25600, 1.25), (76544, 1.0 / 3.0), (76544, 3.7), (711200, 0.93)])
def test_yardstick_is_the_textbook_modulo_a_turn(T, rate):
    """the definition of include/psnd.h never mentions n_fft or hop; the textbook does.  Relative to the case's largest magnitude, on
    STFTs of the seeded_wav recipe: at most 4e-11 for rows up to about 300 frames, 8.4e-9 at 2779 frames (a prototype's figures; the
    textbook's own cumsum of large angles is the limit there)."""
    n_fft, hop = 1024, 256
    re, im = _stft_of(seeded_wav(11, 1, T)[0], n_fft, hop)
    F = re.shape[1]
    tr, ti = R.pv_textbook(re, im, rate, n_fft, hop)
    keep = np.arange(0, 513, 37) if F > 400 else np.arange(0, 513, 8)           # the loop yardstick is slow: a comb of bins, both edges in
    keep = np.union1d(keep, [512])
    J = min(tr.shape[1], R.frames(F, rate))
    yr, yi = R.pv(re[keep], im[keep], rate)
    err = R.rel_err((yr[:, :J], yi[:, :J]), (tr[keep, :J], ti[keep, :J]))
    print('F = %d, rate %g: yardstick against the textbook %.3g' % (F, rate, err))
    assert abs(tr.shape[1] - R.frames(F, rate)) <= 1 and J > 0.9 * F / rate
    assert err <= 1e-7


# ---- known answers --------------------------------------------------------------------------------------------------------------------------
def test_rate_one_is_the_identity():
    K = _K()
    re, im = R.seeded_spectrum(1, 7, 300, seed=3)
    for fn in (lambda a, b: K.phase_vocoder_host(a, b, 1.0), lambda a, b: R.pv(a, b, 1.0)):
        yr, yi = fn(re, im)
        err = R.rel_err((yr, yi), (re, im))
        print('rate 1: %.3g' % err)
        assert yr.shape == re.shape and err <= 1e-12


@pytest.mark.parametrize('rate', (0.5, 0.75, 1.0 / 3.0, 1.3, 1.5, 2.0))
def test_rotating_rows_in_closed_form(rate):
    """X[f] = A e^{i (theta + 2 pi nu hop f / n)} comes out as A e^{i (theta + 2 pi nu hop j / n)} on every output frame with i_j + 1 < F,
    for ARBITRARY nu: the expected advance of the textbook wording cancels modulo a turn"""
    K = _K()
    rs = np.random.RandomState(7)
    rows, F, n, hop = 9, 120, 1024, 256
    A, theta, nu = rs.uniform(0.1, 3.0, (rows, 1)), rs.uniform(-np.pi, np.pi, (rows, 1)), rs.uniform(0.0, 512.0, (rows, 1))
    f = np.arange(F)
    X = A * np.exp(1j * (theta + 2.0 * np.pi * nu * hop * f / n))
    for fn in (K.phase_vocoder_host, R.pv):
        yr, yi = fn(X.real, X.imag, rate)
        j = np.arange(yr.shape[1])
        inner = np.floor(j * rate).astype(int) + 1 < F
        want = A * np.exp(1j * (theta + 2.0 * np.pi * nu * hop * j / n))
        err = R.rel_err((yr[:, inner], yi[:, inner]), (want.real[:, inner], want.imag[:, inner]))
        print('rate %g: closed form %.3g over %d of %d frames' % (rate, err, inner.sum(), inner.size))
        assert inner.sum() >= yr.shape[1] - 3 and err <= 1e-10


# ---- helpers --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.lib()


def test_pv_frames_counts(lib):
    K = _K()
    for rate in (1.0, 0.5, 2.0, 1.0 / 3.0, 0.1, 3.7, 0.93, 0.03, 40.0, 0.7, 1e-3, 2.0 ** -20, 1e6):
        for F in (0, 1, 2, 3, 10, 37, 100, 257, 1000):
            if F / rate > 3e6:
                continue
            want = R.frames(F, rate)
            assert K.pv_frames(F, rate) == want == lib.psnd_pv_frames(F, rate), (F, rate)
    off = [(F, r) for r in (1.0 / 3.0, 0.1, 0.7, 1.0 / 49.0) for F in range(1, 400) if R.frames(F, r) != math.ceil(F / r)]
    print('cases where a bare ceil(F / rate) is wrong:', off[:6])
    for F, r in off:
        assert K.pv_frames(F, r) == R.frames(F, r) == lib.psnd_pv_frames(F, r)
    assert K.pv_frames(-5, 1.0) == 0 and lib.psnd_pv_frames(-5, 1.0) == 0
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert lib.psnd_pv_frames(100, bad) == 0
        with pytest.raises(ValueError):
            K.pv_frames(100, bad)
    assert lib.psnd_pv_frames(100, 1e-300) == 2 ** 63 - 1


def test_pitch_ratio_table():
    K = _K()
    table = {0: (1, 1), 1: (196, 185), -1: (185, 196), 2: (55, 49), 3: (44, 37), 4: (635, 504), 7: (442, 295), 12: (2, 1), -12: (1, 2),
             0.5: (281, 273)}
    for n, want in table.items():
        p, q = K.pitch_ratio(n)
        cents = 1200.0 * abs(math.log2(p / q) - n / 12.0)
        assert (p, q) == want and cents <= 0.03 and max(p, q) <= 640, (n, (p, q), cents)
        assert 20 * max(p, q) + 1 <= K.RESAMPLE_MAX_TAPS
    assert K.pitch_ratio(24, 24) == (2, 1) and K.pitch_ratio(2.0, 12.0) == (55, 49)
    # exhaustive, the slow way round
    for n in (2, 7, -5):
        best = min(((abs(math.log2(p / q) - n / 12.0), p, q) for p in range(1, 641) for q in range(1, 641) if math.gcd(p, q) == 1))
        assert K.pitch_ratio(n) == best[1:]
    for kw in (dict(n_steps=math.nan), dict(n_steps=math.inf), dict(n_steps=2, bins_per_octave=0), dict(n_steps=2, bins_per_octave=-12),
               dict(n_steps=200), dict(n_steps=-200)):
        with pytest.raises(ValueError):
            K.pitch_ratio(**kw)


def test_argument_errors_of_the_python_entries():
    K, U = _K(), _U()
    re = torch.zeros(2, 5, 8)
    for bad in (0.0, -1.0, math.nan, math.inf, 'fast', None, True):
        with pytest.raises(ValueError):
            K.phase_vocoder(re, re, bad)
        with pytest.raises(ValueError):
            K.phase_vocoder_host(re.numpy(), re.numpy(), bad)
        with pytest.raises(ValueError):
            U.time_stretch(np.zeros(4000, np.float32), bad)
    with pytest.raises(K.PsndError):
        K.phase_vocoder(re.numpy(), re.numpy(), 1.0)                            # kernels takes tensors
    with pytest.raises(K.PsndError):
        K.phase_vocoder(re, torch.zeros(2, 5, 9), 1.0)
    with pytest.raises(K.PsndError):
        K.phase_vocoder(re, re.double(), 1.0)
    with pytest.raises(K.PsndError):
        K.phase_vocoder(torch.zeros(8), torch.zeros(8), 1.0)
    with pytest.raises(K.PsndError):
        K.phase_vocoder(re.int(), re.int(), 1.0)
    with pytest.raises(K.PsndError):
        K.phase_vocoder(re, re, 1.0, frames=[8, 8, 8])
    with pytest.raises(K.PsndError):
        K.phase_vocoder(re, re, 1.0, frames=[8.0, 8.0])
    with pytest.raises(ValueError):
        K.phase_vocoder_host(re.numpy(), np.zeros((2, 5, 9)), 1.0)
    with pytest.raises(K.PsndError):
        U.time_stretch(np.float32(1.0), 1.0)
    with pytest.raises(K.PsndError):
        U.time_stretch(torch.zeros(4000, dtype=torch.int16), 1.0)
    with pytest.raises(ValueError):
        U.pitch_shift(np.zeros(4000, np.float32), 0, 2)
    with pytest.raises(ValueError):
        U.pitch_shift(np.zeros(4000, np.float32), 22050, math.nan)
    assert 'gradients are out of scope' in K.phase_vocoder.__doc__
    for word in ('unpinned', 'WSOLA', 'phase vocoder', 'torchaudio', 'librosa', 'tempo'):
        assert word.lower() in ' '.join(U.__doc__.lower().split()), word
    assert 'fraction' in U.pitch_shift.__doc__ and 'irrational' in U.pitch_shift.__doc__


# ---- the C ABI, host side -------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_mirrored(lib):
    from pytorch_sound_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'psnd.h')).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for n in ('psnd_pv_frames', 'psnd_pv_pass', 'psnd_phase_vocoder'):
        assert n + '(' in header and hasattr(h, n) and n in _lib.SIGNATURES, n
    P, I, F64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    assert _lib.SIGNATURES['psnd_phase_vocoder'] == (ctypes.c_int, [P, P, I, I, I, P, F64, P, P, I, P])
    assert _lib.SIGNATURES['psnd_pv_frames'] == (ctypes.c_int64, [I, F64])
    assert 'psnd_phase_vocoder' in _lib.LAUNCHABLE and 'psnd_pv_frames' not in _lib.LAUNCHABLE
    assert lib.psnd_version() >= 148
    # the frames per pass are exported as a function: tests/test_cabi.py pins the header's set of macros, so no macro could be added
    assert lib.psnd_pv_pass() == _K().pv_pass() and _K().pv_pass() % 64 == 0 and _K().pv_pass() > 0


def test_bad_arguments_return_e_arg(lib):
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(re=p, im=p, N=1, K=2, F=100, frames=None, rate=0.5, yre=p, yim=p, J=200, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.psnd_phase_vocoder(*[a[k] for k in ok])

    for bad in (0.0, -0.5, math.nan, math.inf, -math.inf):
        assert call(rate=bad) == -1, bad
    assert b'phase_vocoder' in lib.psnd_last_error() and b'rate' in lib.psnd_last_error()
    assert call(J=-1) == -1 and call(J=0) == -1 and call(J=199) == -1           # J too small
    assert b'psnd_pv_frames' in lib.psnd_last_error()
    for F, r in ((21, 0.7), (5, 1.0 / 3.0), (37, 0.1), (100, 3.7)):             # one slot short of the count, also where the product rounds
        assert call(F=F, rate=r, J=R.frames(F, r) - 1) == -1, (F, r)
    assert call(J=2 ** 31) == -1 and call(J=2 ** 40) == -1
    assert call(rate=1e-300) == -1
    assert call(N=-1) == -1 and call(K=-1) == -1 and call(F=-1) == -1
    assert call(re=None) == -1 and call(im=None) == -1 and call(yre=None) == -1 and call(yim=None) == -1
    assert b'null' in lib.psnd_last_error()
    # nothing to do: nothing launched, no pointer looked at
    none = dict(re=None, im=None, yre=None, yim=None)
    assert call(N=0, **none) == 0 and call(K=0, **none) == 0 and call(F=0, J=0, **none) == 0


# ---- the public functions on the host -------------------------------------------------------------------------------------------------------
def _tone(f, sr, T, phase=0.4):
    return (0.5 * np.sin(2.0 * np.pi * f * np.arange(T) / sr + phase)).astype(np.float32)


def _peak(y, n_fft):
    """(peak bin of the rfft magnitude over the interior - beyond n_fft samples from either end -, its length L)"""
    inner = np.asarray(y, np.float64)[n_fft:-n_fft]
    return int(np.abs(np.fft.rfft(inner * np.hanning(inner.size))).argmax()), inner.size


@pytest.mark.parametrize('rate', (0.8, 1.25))
def test_time_stretch_lengths_composition_and_pitch(rate):
    U, K = _U(), _K()
    from pytorch_sound_amd.models.transforms import STFT
    from pytorch_sound_amd.models.sound import TimeStretch
    sr, T = 22050, 12000
    L = int(round(T / rate)) - 2048
    freqs = (453.0 * sr / L, 1132.25 * sr / L)                                  # on a bin of the interior, and a quarter of a bin off one
    x = np.stack([_tone(freqs[0], sr, T), _tone(freqs[1], sr, T, 1.0)])
    y = U.time_stretch(x, rate)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (2, int(round(T / rate)))
    for row, fr in zip(y, freqs):
        peak, L = _peak(row, 1024)
        assert peak == round(fr * L / sr), (peak, fr * L / sr)
    # the three calls
    stft = STFT(1024, 256)
    xt = torch.from_numpy(x)
    re, im = stft.transform_complex(xt)
    z = stft.inverse_complex(*K.phase_vocoder(re, im, rate))
    n = int(round(T / rate))
    z = z[:, :n] if z.shape[1] >= n else torch.nn.functional.pad(z, (0, n - z.shape[1]))
    assert np.array_equal(z.numpy(), y)
    t = U.time_stretch(xt.double(), rate)
    assert t.dtype == torch.float64 and t.shape == (2, n) and not t.requires_grad
    assert np.abs(t.numpy() - y)[:, 1024:-1024].max() < 1e-5        # the last frames divide by a vanishing overlap-add envelope: left out
    assert U.time_stretch(xt[0], rate).shape == (n,) and U.time_stretch(xt.reshape(2, 1, 1, T), rate).shape == (2, 1, 1, n)
    m = TimeStretch(rate)
    assert np.array_equal(m(xt).numpy(), y) and m(xt[:, None]).shape == (2, 1, n)
    with pytest.raises(RuntimeError):
        m(xt[0])
    for T2, hop in ((5000, 256), (5001, 100), (700, 64)):
        assert U.time_stretch(np.zeros(T2, np.float32), rate, 256, hop).shape == (int(round(T2 / rate)),)


@pytest.mark.parametrize('n_steps', (2, -2, 7))
def test_pitch_shift_length_and_peak(n_steps):
    U, K = _U(), _K()
    from pytorch_sound_amd.models.sound import PitchShift
    sr, T = 22050, 20000                                # the three shifted peaks lie 0.09, 0.15 and 0.27 of a bin from a bin's centre
    x = _tone(440.0, sr, T)
    y = U.pitch_shift(x, sr, n_steps)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (T,)
    p, q = K.pitch_ratio(n_steps)
    peak, L = _peak(y, 1024)
    assert peak == round(440.0 * (p / q) * L / sr), (peak, 440.0 * (p / q) * L / sr)
    xt = torch.from_numpy(x)[None]
    m = PitchShift(sr, n_steps)
    assert (m.p, m.q) == (p, q) and not list(m.parameters()) and 'taps' not in m.state_dict()
    assert np.array_equal(m(xt).numpy()[0], y)
    z = K.resample_poly(U.time_stretch(xt, q / p), q, p)
    z = z[:, :T] if z.shape[1] >= T else torch.nn.functional.pad(z, (0, T - z.shape[1]))
    assert np.array_equal(z.numpy()[0], y)


def test_alias_package_sees_the_new_names():
    import pytorch_sound.utils.sound as a
    import pytorch_sound.models.sound as b
    assert callable(a.time_stretch) and callable(a.pitch_shift) and hasattr(b, 'TimeStretch') and hasattr(b, 'PitchShift')
