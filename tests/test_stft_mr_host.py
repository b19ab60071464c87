"""Host side of the mixed-radix STFT (psnd_stft_mr_*): which sizes are covered, what the plan holds, and that every entry point rejects bad
arguments before it touches the device.  Runs without a GPU."""
import ctypes
import os

import numpy as np
import pytest

from oracle import features as ofe

COVERED = [48, 80, 240, 400, 600, 1200, 4000, 3072]
UNCOVERED = [1024, 1001, 14, 4098, 5000, 2 * 7 * 8]
MAGIC = 0x3152464d


@pytest.fixture(scope='module')
def L():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib


def test_covered_sizes(L):
    lib = L.lib()
    for n in COVERED:
        assert lib.psnd_stft_mr_plan_bytes(n) == 4 * (16 + 3 * n) > 0, n
        assert L.stft_mr_covered(n)
    for n in UNCOVERED:
        assert lib.psnd_stft_mr_plan_bytes(n) == 0, n
        assert not L.stft_mr_covered(n)
    # the power-of-two entry points keep their sizes to themselves (tests/test_cabi.py pins the same)
    assert lib.psnd_stft_plan_bytes(1000) == 0 and lib.psnd_stft_plan_bytes(1200) == 0
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.psnd_stft_fwd(p, 1, 5000, 1000, 256, 0, p, 0.0, p, None, None, None, None) == -4


@pytest.mark.parametrize('n,win', [(240, 200), (1200, 1000), (400, None), (3072, None)])
def test_plan_contents(L, n, win):
    w = ofe.analysis_window(n, win)
    plan = L.build_stft_mr_plan(n, w)
    assert plan.dtype == np.uint8 and plan.nbytes == L.lib().psnd_stft_mr_plan_bytes(n)
    hd = plan[:64].view(np.int32)
    assert hd[0] == MAGIC and hd[1] == n
    P = int(hd[2])
    radices = [int(r) for r in hd[3:3 + P]]
    assert 1 <= P <= 13 and set(radices) <= {2, 3, 4, 5} and int(np.prod(radices)) == n
    assert not hd[3 + P:].any()
    # the documented order: every 5, every 3, every 4, at most one 2 at the end
    rank = {5: 0, 3: 1, 4: 2, 2: 3}
    assert [rank[r] for r in radices] == sorted(rank[r] for r in radices) and radices.count(2) <= 1
    pf = plan.view(np.float32)
    assert np.array_equal(pf[16:16 + n], w)                                   # the window, bit for bit
    tw = pf[16 + n:].reshape(n, 2)
    th = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
    for got, want in ((tw[:, 0], np.cos(th)), (tw[:, 1], -np.sin(th))):
        want32 = want.astype(np.float32)
        # within one fp32 ulp of the correctly rounded float64 value (ulp of the value's own binade; exact zero for a zero of ~1e-16)
        ulp = np.spacing(np.maximum(np.abs(want32), np.float32(1e-30)))
        assert np.all(np.abs(got.astype(np.float64) - want32.astype(np.float64)) <= np.maximum(ulp, 2e-16))


def test_plan_builder_errors(L):
    w = ofe.analysis_window(1200)
    with pytest.raises(L.PsndError):
        L.build_stft_plan(1200, w)                                            # the power-of-two builder is as it was
    with pytest.raises(L.PsndError):
        L.build_stft_mr_plan(1024, ofe.analysis_window(1024))
    with pytest.raises(L.PsndError):
        L.build_stft_mr_plan(1200, w[:-1])
    lib = L.lib()
    out = np.zeros(64, np.uint8)
    assert lib.psnd_stft_mr_plan_build(1200, None, L.np_ptr(out)) == -1
    assert lib.psnd_stft_mr_plan_build(1001, L.np_ptr(w), L.np_ptr(out)) == -4


def test_plan_kind_dispatch(L):
    from pytorch_sound_amd import kernels as K
    p2 = K.stft_plan(1024, ofe.analysis_window(1024))
    pm = K.stft_plan(1200, ofe.analysis_window(1200))
    assert p2.psnd_plan_kind == K.PLAN_POW2 and K.stft_plan_kind(p2, 1024) == K.PLAN_POW2
    assert pm.psnd_plan_kind == K.PLAN_MR and K.stft_plan_kind(pm, 1200) == K.PLAN_MR
    assert K.stft_plan_kind(pm.clone(), 1200) == K.PLAN_MR                    # a copy (Module.to) loses the attribute, not the kind
    assert p2.numel() == L.lib().psnd_stft_plan_bytes(1024) and pm.numel() == L.lib().psnd_stft_mr_plan_bytes(1200)
    assert np.array_equal(p2.numpy(), L.build_stft_plan(1024, ofe.analysis_window(1024)))
    with pytest.raises(L.PsndError, match='1200'):                            # the message names the covered sizes
        K.stft_plan(401, ofe.analysis_window(401))
    assert not K._msl_fused(1200, 300) and L.lib().psnd_stft_fwd_msl_blocks(6000, 1200, 300) == 0


def test_entry_points_validate_before_touching_the_device(L):
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n, hop, T = 1200, 300, 5000
    pb = lib.psnd_stft_mr_plan_bytes(n)
    fwd = lambda **k: lib.psnd_stft_mr_fwd(*[k.get(a, d) for a, d in (          # noqa: E731
        ('wav', p), ('N', 1), ('T', T), ('n', n), ('hop', hop), ('framing', 0), ('plan', p), ('pb', pb), ('eps', 0.0), ('mag', p),
        ('phase', None), ('re', None), ('im', None), ('stream', None))])
    assert fwd(wav=None) == -1 and b'null' in lib.psnd_last_error()
    assert fwd(plan=None) == -1
    assert fwd(mag=None) == -1                                                 # no output requested
    assert fwd(re=p) == -1                                                     # re without im
    assert fwd(hop=0) == -1 and fwd(hop=-3) == -1
    assert fwd(framing=7) == -1
    assert fwd(T=n // 2) == -2                                                 # T <= reflect pad
    assert fwd(T=(n - hop) // 2, framing=1) == -2
    assert fwd(pb=pb - 4) == -1 and fwd(pb=lib.psnd_stft_plan_bytes(1024)) == -1 and fwd(pb=lib.psnd_stft_mr_plan_bytes(400)) == -1
    assert b'plan' in lib.psnd_last_error()
    for bad in (1024, 1001, 14, 4098):
        assert fwd(n=bad, pb=0) == -4
    assert fwd(N=0) == 0                                                       # nothing to do

    sb = lib.psnd_stft_mr_bwd_scratch_bytes(1, T, n, hop, 0)
    assert sb == 4 * ofe.frame_count(T, n, hop, 0) * n
    assert lib.psnd_stft_mr_bwd_scratch_bytes(1, T, 1024, hop, 0) == 0 and lib.psnd_stft_mr_bwd_scratch_bytes(1, T, n, 0, 0) == 0
    bwd = lambda **k: lib.psnd_stft_mr_bwd(*[k.get(a, d) for a, d in (          # noqa: E731
        ('wav', p), ('N', 1), ('T', T), ('n', n), ('hop', hop), ('framing', 0), ('plan', p), ('pb', pb), ('eps', 0.0), ('gmag', p),
        ('gre', None), ('gim', None), ('scratch', p), ('sb', sb), ('gwav', p), ('stream', None))])
    assert bwd(plan=None) == -1 and bwd(gwav=None) == -1
    assert bwd(gmag=None) == -1                                                # no gradient source
    assert bwd(gre=p) == -1                                                    # gre without gim
    assert bwd(wav=None) == -1                                                 # gmag needs the waveform
    assert bwd(hop=0) == -1 and bwd(framing=-1) == -1
    assert bwd(T=n // 2) == -2
    assert bwd(pb=pb + 4) == -1
    assert bwd(scratch=None) == -1 and bwd(sb=sb - 4) == -1 and b'scratch' in lib.psnd_last_error()
    assert bwd(n=1024, pb=lib.psnd_stft_plan_bytes(1024)) == -4
    assert bwd(N=0) == 0

    F = 9
    ib = lib.psnd_istft_mr_scratch_bytes(2, F, n)
    assert ib == 4 * 2 * F * n and lib.psnd_istft_mr_scratch_bytes(2, F, 1024) == 0
    inv = lambda **k: lib.psnd_istft_mr(*[k.get(a, d) for a, d in (             # noqa: E731
        ('mag', p), ('phase', p), ('N', 2), ('F', F), ('n', n), ('hop', hop), ('plan', p), ('pb', pb), ('eps', 0.0), ('scratch', p),
        ('sb', ib), ('out', p), ('stream', None))])
    assert inv(mag=None) == -1 and inv(phase=None) == -1 and inv(plan=None) == -1 and inv(out=None) == -1
    assert inv(hop=0) == -1 and inv(F=-1) == -1
    assert inv(pb=pb - 4) == -1
    assert inv(scratch=None) == -1 and inv(sb=ib - 4) == -1
    assert inv(n=2048, pb=lib.psnd_stft_plan_bytes(2048)) == -4
    assert inv(N=0) == 0 and inv(F=1) == 0                                     # no sample to write


def test_loss_size_gate():
    """multi_stft_loss keeps refusing n_fft = 1000 (tests/test_gpu_sound.py pins it): of the mixed-radix sizes it takes the multiples of
    16; the message names the covered sizes"""
    from pytorch_sound_amd import _lib
    from pytorch_sound_amd import kernels as K
    assert all(K.msl_covered(n) for n in (16, 1024, 8192, 48, 80, 240, 400, 1200, 2400, 3072, 4000))
    assert not any(K.msl_covered(n) for n in (1000, 600, 401, 686, 14, 4098, 5000))
    K.msl_check([1024, 1200, 400])
    with pytest.raises(_lib.PsndError, match='n_fft=600 .*multiples of 16'):
        K.msl_check([1024, 600])
