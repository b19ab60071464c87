"""Separation metrics without a GPU: known answers, the float64 numpy restatement (kernels.sep_metric_host) against the two-pass yardstick
tests/sep_ref.py on every input the GPU tests use - together with the two conditions those tests rely on: every yardstick value lies
below the 60 dB cap of the 1e-4 dB bound, and wherever a permutation is searched the best and the second-best sums are more than 1e-3 dB
apart (the planted tie is decided by rule) - utils.metrics and utils.sound.add_noise on numpy arrays and CPU tensors, and the host side
of the C ABI (declared, exported, bound; bad arguments; helpers)."""
import ctypes
import functools
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sep_ref as R  # noqa: E402
from conftest import ROOT  # noqa: E402

from pytorch_sound_amd import kernels as K  # noqa: E402
from pytorch_sound_amd.utils import metrics as M  # noqa: E402
from pytorch_sound_amd.utils import sound as U  # noqa: E402


def tones(T=4800):
    """two sines of a whole number of periods: orthogonal over the row"""
    t = np.arange(T) / T
    return np.sin(2.0 * math.pi * 5 * t), np.sin(2.0 * math.pi * 9 * t)


@pytest.mark.parametrize('want', [0.0, 6.0, 20.0, 40.0])
def test_orthogonal_noise_at_a_chosen_ratio_reads_that_snr(want):
    s, n = tones()
    e = s + 10.0 ** (-want / 20.0) * n
    for kind in R.KINDS:                                 # <e, s> = <s, s>: the scale a is 1 and the three coincide
        for zm in (False, True):
            got = K.sep_metric_host(e[None, None], s[None, None], kind, zm, eps=0.0).item()
            assert abs(got - want) <= 1e-4, (kind, zm, got)
    assert abs(float(M.snr(e.astype(np.float32), s.astype(np.float32))) - want) <= 1e-3


def test_scale_invariance_and_the_relations_between_the_three():
    rs = np.random.RandomState(1)
    s = rs.randn(3, 4000)
    e = 0.5 * s + 0.2 * rs.randn(3, 4000)                # a downscaled estimate: a < 1
    get = lambda kind, est: K.sep_metric_host(est[:, None], s[:, None], kind, False, eps=0.0).astype(np.float64)[:, 0]  # noqa: E731
    for c in (0.1, 3.0, -2.0):
        assert np.allclose(get('si_sdr', c * e), get('si_sdr', e), rtol=0, atol=1e-4)
        assert np.all(np.abs(get('snr', c * e) - get('snr', e)) > 0.5)
    snr, si, sd = get('snr', e), get('si_sdr', e), get('sd_sdr', e)
    a = (e * s).sum(-1) / (s * s).sum(-1)
    assert np.all(a < 1.0)
    assert np.allclose(sd, snr + 10.0 * np.log10(a * a), rtol=0, atol=1e-4)      # SD-SDR = SNR + 10 log10 a^2 (Le Roux et al., eq. 6)
    assert np.all(sd <= si + 1e-6) and np.all(sd <= snr + 1e-6)                  # the projection is the closest scaled target; a < 1
    up = get('sd_sdr', 4.0 * e)                                                  # a > 1: SD-SDR can exceed the SNR, never SI-SDR
    assert np.all(up <= get('si_sdr', 4.0 * e) + 1e-6) and np.all(up > get('snr', 4.0 * e))
    # zero_mean takes a DC offset out: without it the offset counts as signal
    d = e + 3.0
    zm = K.sep_metric_host(d[:, None], (s + 3.0)[:, None], 'si_sdr', True)[:, 0]
    assert np.allclose(zm, K.sep_metric_host(e[:, None], s[:, None], 'si_sdr', True)[:, 0], rtol=0, atol=1e-3)
    assert np.all(K.sep_metric_host(d[:, None], (s + 3.0)[:, None], 'si_sdr', False)[:, 0] > zm + 3.0)


@functools.lru_cache(maxsize=None)
def _readings(name):
    est, tgt, lens, pit = R.case(name)
    configs = R.CONFIGS if name != 'full' else R.FULL_CONFIGS
    return est, tgt, lens, pit, {c: R.measure(est, tgt, c[0], c[1], lengths=lens, pit=pit) for c in configs}


@pytest.mark.parametrize('name', R.CASES)
def test_gpu_inputs_stay_under_the_cap_and_clear_of_permutation_ties(name):
    est, tgt, lens, pit, readings = _readings(name)
    for (kind, zm), r in readings.items():
        top = float(np.nanmax(r.value))
        print('%s %s zero_mean=%d: largest value %.2f dB, permutation gap %.3g dB' % (name, kind, zm, top, r.gap))
        assert top <= R.CAP_DB and float(np.nanmax(r.pair)) <= R.CAP_DB
        if pit and name != 'tie':
            assert r.gap > R.GAP_DB
    if name == 'tie':                                    # decided by rule: the lexicographically first of the two best, identity for no samples
        r = readings[('snr', False)]
        assert r.gap == 0.0 and r.perm.tolist() == [[1, 2, 0], [0, 1, 2]]
    if name == 'pit3':
        assert readings[('si_sdr', True)].perm.tolist() == R.S3_PERMS
    if name == 'pit4':
        assert readings[('si_sdr', True)].perm.tolist() == R.S4_PERM


@pytest.mark.parametrize('name', R.CASES)
def test_host_equals_the_yardstick(name):
    est, tgt, lens, pit, readings = _readings(name)
    for (kind, zm), r in readings.items():
        value, perm, pair = K.sep_metric_host(est, tgt, kind, zm, None, lens, pit, True, True)
        assert value.dtype == np.float32 and perm.dtype == np.int32 and pair.dtype == np.float32
        assert value.shape == est.shape[:2] and pair.shape == est.shape[:2] + est.shape[1:2]
        assert np.array_equal(perm, r.perm)
        assert float(np.max(np.abs(value - r.value))) <= 1e-5 and float(np.max(np.abs(pair - r.pair))) <= 1e-5, (kind, zm)


def test_the_high_ratio_case_is_near_100_db():
    est, tgt = R.high_ratio_case()
    for kind, zm in R.CONFIGS:
        v = R.measure(est, tgt, kind, zm).value.item()
        assert 95.0 < v < 105.0
        assert abs(K.sep_metric_host(est, tgt, kind, zm).item() - v) <= R.moment_bound_db(v, 1)
    # what the derivation gives: a row of 30 s at 44.1 kHz has m + d = 162 + 42; the 1e-4 dB bound leaves a factor of ten at the cap
    assert R.moment_bound_db(100.0, 50) < 2e-3 and R.moment_bound_db(R.CAP_DB, 300) < 1e-5


def test_non_finite_items_lengths_and_bad_arguments():
    est, tgt = R.sources(5, 3, 2, 500)
    base = K.sep_metric_host(est, tgt, 'si_sdr', True, pit=True, return_perm=True)
    bad = est.copy()
    bad[1, 0, 7] = np.nan
    value, perm = K.sep_metric_host(bad, tgt, 'si_sdr', True, pit=True, return_perm=True)
    assert np.isnan(value[1]).all() and perm[1].tolist() == [0, 1]
    assert np.array_equal(value[[0, 2]], base[0][[0, 2]]) and np.array_equal(perm[[0, 2]], base[1][[0, 2]])
    cut = K.sep_metric_host(bad, tgt, 'si_sdr', True, lengths=[500, 7, 300])      # the NaN lies behind the length
    assert np.isfinite(cut).all() and np.array_equal(cut[1], K.sep_metric_host(est[1:2, :, :7], tgt[1:2, :, :7], 'si_sdr', True)[0])
    assert np.array_equal(K.sep_metric_host(est, tgt, 'snr', lengths=[0, 0, 0]), np.zeros((3, 2), np.float32))   # eps / eps
    with pytest.raises(ValueError):
        K.sep_metric_host(est, tgt, 'sdr')
    with pytest.raises(ValueError):
        K.sep_metric_host(est, tgt, 'snr', eps=-1.0)
    with pytest.raises(K.PsndError):
        K.sep_metric_host(est, tgt[:, :1], 'snr')
    with pytest.raises(K.PsndError):
        K.sep_metric_host(est, tgt, 'snr', lengths=[1, 2])


@pytest.mark.parametrize('box', ['numpy', 'cpu_tensor'])
def test_public_metrics_on_the_host(box):
    est, tgt = R.sources(9, 4, 3, 1200, perms=[[0, 1, 2], [2, 0, 1], [1, 0, 2], [0, 2, 1]])
    wrap = (lambda a: a) if box == 'numpy' else (lambda a: torch.from_numpy(np.array(a)))
    unwrap = (lambda a: a) if box == 'numpy' else (lambda a: a.numpy())
    for fn, kind, zm in ((M.snr, 'snr', False), (M.si_sdr, 'si_sdr', True), (M.sd_sdr, 'sd_sdr', False)):
        got = fn(wrap(est), wrap(tgt))                   # any leading shape, rows matched as given, the torchmetrics defaults
        assert type(got) is type(wrap(est)) and tuple(got.shape) == (4, 3) and unwrap(got).dtype == np.float32
        want = np.array([[R.pair_value(kind, est[b, i].astype(np.float64), tgt[b, i].astype(np.float64), zm) for i in range(3)] for b in range(4)])
        assert float(np.max(np.abs(unwrap(got) - want))) <= 1e-5
        one = fn(wrap(est[0, 0]), wrap(tgt[0, 0]))
        assert tuple(one.shape) == () and abs(float(one) - want[0, 0]) <= 1e-5
        cut = fn(wrap(est[:, 0]), wrap(tgt[:, 0]), lengths=[1200, 600, 1, 0])
        assert abs(float(cut[1]) - R.pair_value(kind, est[1, 0, :600].astype(np.float64), tgt[1, 0, :600].astype(np.float64), zm)) <= 1e-5
    values, perm = M.pit(wrap(est), wrap(tgt))
    ref = R.measure(est, tgt, 'si_sdr', True, pit=True)
    assert unwrap(perm).tolist() == ref.perm.tolist() == [[0, 1, 2], [2, 0, 1], [1, 0, 2], [0, 2, 1]]
    assert float(np.max(np.abs(unwrap(values) - ref.value))) <= 1e-5
    lined = M.permute_sources(wrap(tgt), perm)           # the targets in the order of the estimates
    assert type(lined) is type(wrap(tgt))
    assert np.array_equal(unwrap(lined), np.stack([tgt[b, ref.perm[b]] for b in range(4)]))
    assert float(np.max(np.abs(unwrap(M.si_sdr(wrap(est), lined)) - ref.value))) <= 1e-5
    snr_values, _ = M.pit(wrap(est), wrap(tgt), kind='snr')
    assert float(np.max(np.abs(unwrap(snr_values) - R.measure(est, tgt, 'snr', False, pit=True).value))) <= 1e-5


@pytest.mark.parametrize('box', ['numpy', 'cpu_tensor'])
def test_add_noise_reaches_the_asked_snr(box):
    rs = np.random.RandomState(3)
    wav = (0.1 * rs.randn(4, 3000)).astype(np.float32)
    noise = (0.7 * rs.randn(4, 3000)).astype(np.float32)
    wav[2] = 0.0                                         # silent speech: unchanged
    noise[3, 5] = np.inf                                 # a non-finite row: unchanged
    snr = np.array([20.0, -5.0, 10.0, 10.0], dtype=np.float32)
    wrap = (lambda a: a) if box == 'numpy' else (lambda a: torch.from_numpy(np.array(a)))
    y = U.add_noise(wrap(wav), wrap(noise), wrap(snr))
    y = y if box == 'numpy' else y.numpy()
    assert y.dtype == np.float32 and y.shape == wav.shape
    want, gain = R.mix(wav, noise, snr)
    assert float(np.max(np.abs(y - want))) <= 1e-6 and gain[2] == 0.0 and gain[3] == 0.0
    assert np.array_equal(y[2], wav[2]) and np.array_equal(y[3], wav[3])
    got = M.snr(y[:2], wav[:2])                          # the mixture as the estimate of the clean signal
    assert abs(float(got[0]) - 20.0) <= 1e-3 and abs(float(got[1]) + 5.0) <= 1e-3
    y = U.add_noise(wrap(wav), wrap(noise), 15.0, lengths=[3000, 1000, 3000, 3000])
    y = y if box == 'numpy' else y.numpy()
    assert np.array_equal(y[1, 1000:], wav[1, 1000:]) and abs(float(M.snr(y[1, :1000], wav[1, :1000])) - 15.0) <= 1e-3
    assert abs(float(M.snr(y[0], wav[0])) - 15.0) <= 1e-3
    silent = U.add_noise(wrap(wav[:1]), wrap(np.zeros((1, 3000), np.float32)), 0.0)
    assert np.array_equal(silent if box == 'numpy' else silent.numpy(), wav[:1])
    if box == 'cpu_tensor':
        with pytest.raises(K.PsndError):
            U.add_noise(torch.from_numpy(wav).requires_grad_(True), torch.from_numpy(noise), 10.0)
        assert U.add_noise(torch.from_numpy(wav).double(), torch.from_numpy(noise).double(), 10.0).dtype == torch.float64
    with pytest.raises(K.PsndError):
        U.add_noise(wrap(wav), wrap(noise[:2]), 10.0)
    with pytest.raises(K.PsndError):
        U.add_noise(wrap(wav), wrap(noise), [1.0, 2.0])


def test_the_module_and_the_alias_package():
    import pytorch_sound.utils.metrics as alias
    import pytorch_sound.models.sound as alias_models
    from pytorch_sound_amd.models.sound import SeparationLoss
    assert alias is M and alias_models.SeparationLoss is SeparationLoss
    loss = SeparationLoss()
    assert (loss.kind, loss.pit, loss.zero_mean) == ('si_sdr', False, True) and SeparationLoss('snr').zero_mean is False
    assert SeparationLoss('sd_sdr', pit=True, zero_mean=True).zero_mean is True and 'pit=True' in repr(SeparationLoss(pit=True))
    with pytest.raises(ValueError):
        SeparationLoss('sdr')
    with pytest.raises(ValueError):
        SeparationLoss(eps=-1.0)
    with pytest.raises(RuntimeError, match='HIP'):       # no quiet host fall-back for the training loss
        loss(torch.zeros(2, 2, 100), torch.zeros(2, 2, 100))
    with pytest.raises(RuntimeError):
        loss(torch.zeros(2, 100), torch.zeros(2, 99))


# ---- the C ABI, host side -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib.lib()


NAMES = ('psnd_sep_span', 'psnd_sep_max_sources', 'psnd_sep_scratch_bytes', 'psnd_sep_stats_doubles', 'psnd_sep_metric_fwd',
         'psnd_sep_metric_bwd', 'psnd_snr_gain', 'psnd_mix_rows')
PINNED_MACROS = 26          # tests/test_cabi.py pins the header's integer macros by name: the kinds are plain ints, no macro is added


def test_entries_are_declared_exported_and_bound(lib):
    from pytorch_sound_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'psnd.h')).read()
    h = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert n + '(' in header and hasattr(h, n) and n in _lib.SIGNATURES, n
    for n in NAMES[4:]:
        assert n in _lib.LAUNCHABLE and callable(getattr(_lib.on, n))
    for n in NAMES[:4]:
        assert n not in _lib.LAUNCHABLE
    assert len(_lib.SIGNATURES['psnd_sep_metric_fwd'][1]) == 18 and len(_lib.SIGNATURES['psnd_sep_metric_bwd'][1]) == 15
    assert lib.psnd_version() >= 152
    assert not [m for m in _lib.DEFINES if 'SEP' in m or 'SNR' in m or 'SDR' in m]
    stripped = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert len(re.findall(r'^#define (PSND_\w+) \(?(-?\d+)\)?\s*$', stripped, flags=re.M)) == PINNED_MACROS
    for word in ('mir_eval', 'PESQ', 'Hungarian', 'multichannel'):      # what is out of scope is said where the definition is
        assert word in header


def test_helpers_return_what_the_header_says(lib):
    assert lib.psnd_sep_span() == R.SPAN == K.sep_span()
    assert lib.psnd_sep_max_sources() >= 4 and lib.psnd_sep_max_sources() == K.sep_max_sources()
    for B, S in ((1, 1), (3, 2), (5, 3), (7, 4)):
        assert lib.psnd_sep_stats_doubles(B, S) == B * (S * S + 4 * S + 2)
        for T in (1, R.SPAN, R.SPAN + 1, 100000):
            assert lib.psnd_sep_scratch_bytes(B, S, T) == 8 * B * -(-T // R.SPAN) * (S * S + 4 * S + 1), (B, S, T)
    assert lib.psnd_sep_stats_doubles(0, 2) == 0 and lib.psnd_sep_stats_doubles(2, 0) == 0 and lib.psnd_sep_stats_doubles(2, 5) == 0
    assert lib.psnd_sep_scratch_bytes(0, 1, 100) == 0 and lib.psnd_sep_scratch_bytes(1, 1, 0) == 0 and lib.psnd_sep_scratch_bytes(1, 5, 100) == 0


def test_bad_arguments_return_their_codes_before_any_launch(lib):
    buf = (ctypes.c_double * 4096)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    ok = dict(est=p, target=p, B=1, S=2, T=100, lengths=None, kind=1, zero_mean=1, eps=1e-7, pit=1, scratch=p, stats=p, value=p, perm=p,
              pair=None, loss=None, nan_flag=None, stream=None)

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.psnd_sep_metric_fwd(*[a[k] for k in ok])

    assert fwd(kind=3) == -1 and fwd(kind=-1) == -1
    assert b'sep_metric_fwd' in lib.psnd_last_error()
    assert fwd(eps=-1e-9) == -1 and fwd(eps=math.nan) == -1 and fwd(eps=math.inf) == -1
    assert fwd(S=0) == -1 and fwd(S=-3) == -1
    assert fwd(B=-1) == -1 and fwd(T=-1) == -1
    assert fwd(zero_mean=2) == -1 and fwd(pit=2) == -1
    for k in ('est', 'target', 'scratch', 'stats', 'value', 'perm'):
        assert fwd(**{k: None}) == -1, k
    assert fwd(scratch=ctypes.c_void_p(p.value + 4)) == -1
    assert fwd(S=lib.psnd_sep_max_sources() + 1) == -4
    assert fwd(B=2 ** 31, T=8192) == -2
    # nothing to do, nothing launched (no loss asked for: nothing is touched)
    assert fwd(B=0) == 0 and fwd(T=0) == 0 and fwd(B=0, est=None, target=None, scratch=None, stats=None, value=None, perm=None) == 0
    assert fwd(B=0, kind=7) == -1 and fwd(T=0, eps=-1.0) == -1               # the checks come first

    okb = dict(est=p, target=p, B=1, S=2, T=100, kind=1, zero_mean=1, eps=1e-7, stats=p, perm=p, g_loss=p, g_value=None, g_est=p,
               g_target=None, stream=None)

    def bwd(**kw):
        a = dict(okb, **kw)
        return lib.psnd_sep_metric_bwd(*[a[k] for k in okb])

    assert bwd(kind=3) == -1 and bwd(eps=-1.0) == -1 and bwd(eps=math.nan) == -1 and bwd(S=0) == -1 and bwd(B=-1) == -1 and bwd(T=-1) == -1
    assert b'sep_metric_bwd' in lib.psnd_last_error()
    for k in ('est', 'target', 'stats', 'perm', 'g_est'):
        assert bwd(**{k: None}) == -1, k
    assert bwd(g_loss=None, g_value=None) == -1                               # a gradient has to come from somewhere
    assert bwd(S=5) == -4 and bwd(B=2 ** 31) == -2
    assert bwd(B=0) == 0 and bwd(T=0) == 0

    okg = dict(x=p, z=p, R=2, T=100, lengths=None, snr=p, snr_n=2, scratch=p, gain=p, stream=None)

    def gain(**kw):
        a = dict(okg, **kw)
        return lib.psnd_snr_gain(*[a[k] for k in okg])

    assert gain(R=-1) == -1 and gain(T=-1) == -1 and gain(snr_n=3) == -1 and gain(snr_n=0) == -1
    assert b'snr_gain' in lib.psnd_last_error()
    for k in ('x', 'z', 'snr', 'scratch', 'gain'):
        assert gain(**{k: None}) == -1, k
    assert gain(scratch=ctypes.c_void_p(p.value + 4)) == -1
    assert gain(R=2 ** 31, snr_n=1, T=8192) == -2 and gain(R=0, snr_n=1) == 0

    okm = dict(x=p, z=p, R=2, T=100, lengths=None, gain=p, y=p, stream=None)

    def mix(**kw):
        a = dict(okm, **kw)
        return lib.psnd_mix_rows(*[a[k] for k in okm])

    assert mix(R=-1) == -1 and mix(T=-1) == -1
    for k in ('x', 'z', 'gain', 'y'):
        assert mix(**{k: None}) == -1, k
    assert b'mix_rows' in lib.psnd_last_error()
    assert mix(R=2 ** 31) == -2 and mix(R=0) == 0 and mix(T=0) == 0
