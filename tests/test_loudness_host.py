"""Loudness without a GPU: the K-weighting table, the float64 numpy restatement (kernels.loudness_host) against the sequential yardstick
tests/loudness_ref.py, known answers of EBU Tech 3341, the gates, utils.sound.normalize on numpy arrays and CPU tensors, the margin
condition of the inputs the GPU tests use, and the host side of the C ABI (declared, exported, bound; bad arguments; helpers)."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

from pytorch_sound_amd import kernels as K  # noqa: E402
from pytorch_sound_amd.utils import sound as U  # noqa: E402


def sine(sr, seconds=5.0, freq=997.0, amp=1.0):
    return (amp * np.sin(2.0 * math.pi * freq * np.arange(int(seconds * sr)) / sr)).astype(np.float32)


def test_k_weighting_is_the_table_at_48k():
    (b1, a1), (b2, a2) = K.k_weighting(48000)
    assert np.allclose(b1, [1.53512485958697, -2.69169618940638, 1.19839281085285], rtol=0, atol=1e-12)
    assert np.allclose(a1, [1.0, -1.69065929318241, 0.73248077421585], rtol=0, atol=1e-12)
    assert b2 == [1.0, -2.0, 1.0]
    assert np.allclose(a2, [1.0, -1.99004745483398, 0.99007225036621], rtol=0, atol=1e-12)
    for sr in (8000, 16000, 22050, 44100, 48000):
        for (b, a), (rb, ra) in zip(K.k_weighting(sr), R.k_weighting(sr)):
            assert np.allclose(b, rb, rtol=0, atol=1e-14) and np.allclose(a, ra, rtol=0, atol=1e-14)
        assert K.loudness_block(sr) == R.block(sr)
    assert K.loudness_block(8000) == (3200, 800) and K.loudness_block(11025) == (4410, 1102)
    assert K.LOUDNESS_GATE == R.GATE


@pytest.mark.parametrize('sr,want,tol', [(48000, -3.0103, 0.01), (44100, -3.01, 0.1), (22050, -3.01, 0.1), (16000, -3.01, 0.1)])
def test_full_scale_sine_reads_minus_3(sr, want, tol):
    x = sine(sr)
    got = float(K.loudness_host(x, sr))
    print('997 Hz 0 dBFS at %d Hz: %.4f LUFS' % (sr, got))
    assert abs(got - want) <= tol
    assert abs(got - R.measure(x, sr).lufs) <= 1e-5


def test_minus_23_sine():
    x = sine(48000, amp=10.0 ** (-23.0 / 20.0) * math.sqrt(2.0))
    assert abs(float(U.loudness(x, 48000)) + 23.0) <= 0.01


def test_relative_gate_on_the_two_level_sine():
    x = R.two_level_sine()
    got = float(K.loudness_host(x, 16000))
    ref = R.measure(x, 16000)
    print('two-level sine: %.4f LUFS, yardstick %.4f, margin %.3g' % (got, ref.lufs, ref.margin))
    assert abs(got + 9.85) <= 0.01 and abs(got - ref.lufs) <= 1e-5
    ungated = -0.691 + 10.0 * math.log10(float(np.mean(ref.z)))
    assert got > ungated + 2.0
    assert ref.margin > R.MARGIN


def test_silence_short_rows_and_nan():
    sr = 8000
    B, H = K.loudness_block(sr)
    assert float(K.loudness_host(np.zeros(2 * B, dtype=np.float32), sr)) == -math.inf
    x = R.gated_noise(3, B + 3 * H, sr)
    assert float(K.loudness_host(x[:B - 1], sr)) == -math.inf and math.isfinite(float(K.loudness_host(x[:B], sr)))
    rows = np.stack([x, x, x])
    base = K.loudness_host(rows, sr)
    rows[1, B + 7] = np.nan
    got, blocks = K.loudness_host(rows, sr, return_blocks=True)
    assert math.isnan(got[1]) and got[0] == base[0] and got[2] == base[2]
    assert np.isnan(blocks[1]).all() and np.isfinite(blocks[0]).all()
    rows[1, B + 7] = np.inf
    assert math.isnan(K.loudness_host(rows, sr)[1])
    # lengths: what lies behind a programme's length does not enter
    rows[1, B + 7] = np.nan
    got = K.loudness_host(rows, sr, lengths=[B + 3 * H, B + 7, B - 1])
    assert got[0] == base[0] and got[1] == K.loudness_host(x[:B + 7], sr) and got[2] == -math.inf


@pytest.mark.parametrize('name,sr,T,C', R.cases())
def test_host_equals_the_yardstick_and_inputs_keep_clear_of_the_gates(name, sr, T, C):
    x = R.case_input(name, sr, T, C)
    ref = R.measure(x, sr)
    got, blocks = K.loudness_host(x, sr, channels=C, return_blocks=True)
    print('%s sr=%d T=%s C=%s: %.5f LUFS, yardstick %.5f, %d blocks, margin %.3g' % (name, sr, T, C, float(got), ref.lufs, len(ref.z),
                                                                                   ref.margin))
    assert ref.margin > R.MARGIN                         # the condition of the GPU tests, asserted on the yardstick
    if math.isinf(ref.lufs):
        assert float(got) == ref.lufs
    else:
        assert abs(float(got) - ref.lufs) <= 1e-5
    assert blocks.shape == (len(ref.z),) and np.allclose(blocks, ref.z, rtol=1e-6, atol=0)
    if name == 'noise' and T >= 2 * sr:                  # two seconds or more: both gates cut something
        za = ref.z[ref.z > R.GATE]
        assert 0 < za.size < ref.z.size and (za <= 0.1 * za.mean()).any()
    if name == 'loud_quiet':                             # the quiet half is 65 dB below the loud one, not lost in it
        q = ref.z[-4:] / ref.z[:4].mean()
        assert np.all(np.abs(10.0 * np.log10(q) + 65.0) < 1.0)


def test_multichannel_weights():
    sr = 8000
    x = R.gated_noise(5, 9000, sr, 5)
    w = [0.5, 2.0, 1.0, 0.0, 1.25]
    assert abs(float(K.loudness_host(x, sr, channels=5, weights=w)) - R.measure(x, sr, w).lufs) <= 1e-5
    assert abs(float(K.loudness_host(x, sr, channels=5)) - R.measure(x, sr).lufs) <= 1e-5
    batch = np.stack([x, 0.5 * x])
    got = K.loudness_host(batch, sr, channels=5)
    assert got.shape == (2,) and abs(float(got[0] - got[1]) - 20.0 * math.log10(2.0)) <= 1e-4
    with pytest.raises(K.PsndError):
        K.loudness_host(np.zeros((6, 9000), dtype=np.float32), sr, channels=6)
    with pytest.raises(K.PsndError):
        K.loudness_host(x, sr, channels=4)


@pytest.mark.parametrize('kind', ['ebu', 'rms', 'peak'])
@pytest.mark.parametrize('box', ['numpy', 'cpu_tensor'])
def test_normalize_on_the_host(kind, box):
    sr, target = 8000, {'ebu': -23.0, 'rms': -20.0, 'peak': -1.0}[kind]
    x = np.stack([R.gated_noise(1, 9000, sr), np.zeros(9000, dtype=np.float32), 3.0 * R.gated_noise(2, 9000, sr)])
    a = x if box == 'numpy' else torch.from_numpy(x.copy()).double()
    y = U.normalize(a, sr, target, kind)
    if box == 'numpy':
        assert isinstance(y, np.ndarray) and y.dtype == np.float32
    else:
        assert isinstance(y, torch.Tensor) and y.dtype == torch.float64
        y = y.numpy()
    assert y.shape == x.shape and np.array_equal(y[1], x[1])          # a silent row comes back unchanged
    for n in (0, 2):
        got = {'ebu': lambda v: R.measure(v, sr).lufs, 'rms': R.rms_db, 'peak': R.peak_db}[kind](y[n])
        assert abs(got - target) <= 1e-3, (n, got)
    with pytest.raises(ValueError):
        U.normalize(x, sr, target, 'lufs')
    short = R.gated_noise(1, 3199, sr)                                  # one sample short of a block
    assert np.array_equal(U.normalize(short, sr, -23.0, 'ebu'), short)


def test_levels_and_gain_on_the_host():
    x = np.stack([R.gated_noise(1, 5000, 8000), np.zeros(5000, dtype=np.float32)])
    for kind, ref in (('rms', R.rms_db), ('peak', R.peak_db)):
        got = K.level(x, kind)
        assert got.dtype == np.float32 and abs(float(got[0]) - ref(x[0])) <= 1e-4 and got[1] == -math.inf
        assert abs(float(K.level(x, kind, lengths=[1234, 5000])[0]) - ref(x[0, :1234])) <= 1e-4
    g = K.gain_of_level(np.array([-20.0, -math.inf, math.nan], dtype=np.float32), -14.0)
    assert g.dtype == np.float32 and abs(g[0] - 10.0 ** 0.3) < 1e-6 and g[1] == 1.0 and g[2] == 1.0
    y = K.apply_gain(x, [2.0, 3.0], lengths=[100, 5000])
    assert np.array_equal(y[0, :100], 2.0 * x[0, :100]) and np.array_equal(y[0, 100:], x[0, 100:])
    from pytorch_sound_amd.models.sound import LoudnessNorm
    mod = LoudnessNorm(8000, -20.0, 'rms')
    out = mod(torch.from_numpy(x[:1].copy()))
    assert abs(R.rms_db(out[0].numpy()) + 20.0) <= 1e-3 and 'rms' in repr(mod)
    with pytest.raises(ValueError):
        LoudnessNorm(8000, kind='true_peak')


# ---- the C ABI, host side -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.lib()


NAMES = ('psnd_loudness_span', 'psnd_loudness_max_channels', 'psnd_loudness_blocks', 'psnd_loudness_scratch_bytes', 'psnd_loudness',
         'psnd_row_level', 'psnd_gain_rows')
PINNED_MACROS = 26          # tests/test_cabi.py pins the header's integer macros by name: the new entry points add none


def test_entries_are_declared_exported_and_bound(lib):
    from pytorch_sound_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'psnd.h')).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + '(' in header and hasattr(h, n) and n in _lib.SIGNATURES, n
    for n in ('psnd_loudness', 'psnd_row_level', 'psnd_gain_rows'):
        assert n in _lib.LAUNCHABLE and callable(getattr(_lib.on, n))
    assert len(_lib.SIGNATURES['psnd_loudness'][1]) == 24
    assert lib.psnd_version() >= 151
    assert not [m for m in _lib.DEFINES if 'LOUD' in m or 'LEVEL' in m or 'GAIN' in m]
    stripped = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert len(re.findall(r'^#define (PSND_\w+) \(?(-?\d+)\)?\s*$', stripped, flags=re.M)) == PINNED_MACROS


def test_helpers_return_what_the_definition_says(lib):
    assert lib.psnd_loudness_span() == R.SPAN == K.loudness_span()
    assert lib.psnd_loudness_max_channels() >= 5
    for T in (0, 1, 3199, 3200, 3999, 4000, 4001, 8191, 8192, 100000):
        for B, H in ((3200, 800), (4410, 1102), (7, 3), (5, 5), (1, 1)):
            assert lib.psnd_loudness_blocks(T, B, H) == R.n_blocks(T, B, H) == K.loudness_blocks(T, B, H), (T, B, H)
    assert lib.psnd_loudness_blocks(100, 0, 1) == 0 and lib.psnd_loudness_blocks(100, 10, 0) == 0
    # scratch: per (row, span) a carry of four doubles, a flag, and a double per piece of a span (hops of H, cut again where H does not divide B)
    for N, C, T, B, H in ((1, 1, 8192, 3200, 800), (3, 2, 8193, 3200, 800), (2, 1, 40000, 4410, 1102), (1, 5, 100, 7, 1)):
        rs = N * C * -(-T // 8192)
        pieces = (2 if B % H else 1) * (8192 // H + 2)
        got = lib.psnd_loudness_scratch_bytes(N, C, T, B, H)
        assert rs * (32 + 4 + 8 * pieces) <= got <= rs * (32 + 4 + 8 * pieces) + 48, (N, C, T, B, H, got)
    assert lib.psnd_loudness_scratch_bytes(0, 1, 100, 10, 5) == 0 and lib.psnd_loudness_scratch_bytes(1, 1, 100, 5, 10) == 0


def test_bad_arguments_return_e_arg(lib):
    buf = (ctypes.c_double * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    (b1, a1), (b2, a2) = K.k_weighting(8000)
    ok = dict(x=p, N=1, C=1, T=100, lengths=None, sb0=b1[0], sb1=b1[1], sb2=b1[2], sa1=a1[1], sa2=a1[2], hb0=b2[0], hb1=b2[1], hb2=b2[2],
              ha1=a2[1], ha2=a2[2], B=40, H=10, weights=None, target=-23.0, scratch=p, lufs=p, blocks=None, gain=None, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.psnd_loudness(*[a[k] for k in ok])

    assert call(B=0) == -1 and call(H=0) == -1 and call(H=41) == -1 and call(B=-5, H=-5) == -1
    assert b'loudness' in lib.psnd_last_error()
    assert call(C=0) == -1 and call(C=-2) == -1
    for k in ('sb0', 'sb1', 'sb2', 'sa1', 'sa2', 'hb0', 'hb1', 'hb2', 'ha1', 'ha2'):
        assert call(**{k: math.nan}) == -1 and call(**{k: math.inf}) == -1, k
    assert call(target=math.nan) == -1
    assert call(C=2, weights=(ctypes.c_double * 2)(1.0, math.nan)) == -1 and call(C=2, weights=(ctypes.c_double * 2)(math.inf, 1.0)) == -1
    assert call(C=6) == -1                                              # more than five channels need explicit weights
    assert call(N=-1) == -1 and call(T=-1) == -1
    assert call(x=None) == -1 and call(lufs=None) == -1 and call(scratch=None) == -1
    assert call(scratch=ctypes.c_void_p(p.value + 8)) == -1
    assert call(C=lib.psnd_loudness_max_channels() + 1, weights=p) == -4
    assert call(N=2 ** 31, T=8192) == -2
    assert call(N=0) == 0 and call(T=0) == 0 and call(N=0, x=None, lufs=None, scratch=None) == 0      # nothing to do, nothing launched

    lv = dict(x=p, N=1, C=1, T=100, lengths=None, of_peak=0, target=-20.0, rms_db=p, peak_db=p, gain=p, stream=None)

    def level(**kw):
        a = dict(lv, **kw)
        return lib.psnd_row_level(*[a[k] for k in lv])

    assert level(C=0) == -1 and level(N=-1) == -1 and level(T=-1) == -1 and level(of_peak=2) == -1 and level(target=math.inf) == -1
    assert level(x=None) == -1 and level(rms_db=None, peak_db=None, gain=None) == -1
    assert b'row_level' in lib.psnd_last_error()
    assert level(N=2 ** 31) == -2 and level(N=0) == 0

    gn = dict(x=p, N=1, C=1, T=100, lengths=None, gain=p, y=p, stream=None)

    def gain(**kw):
        a = dict(gn, **kw)
        return lib.psnd_gain_rows(*[a[k] for k in gn])

    assert gain(C=0) == -1 and gain(N=-1) == -1 and gain(T=-1) == -1
    assert gain(x=None) == -1 and gain(y=None) == -1 and gain(gain=None) == -1
    assert gain(N=2 ** 31) == -2 and gain(N=0) == 0 and gain(T=0) == 0
