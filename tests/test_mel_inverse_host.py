"""The mel-inverse section of include/psnd.h without a GPU: kernels.mel_inverse_host against the yardstick tests/melinv_ref.py, the plan
builder of the C ABI against numpy (to the bit) and its error paths, the properties that follow from the definition on CPU tensors, and the
public layers (InverseMelScale, LogMelSpectrogram.inverse_mel, utils.sound.mel_to_magnitude / mel_to_wave, MelToWave, LogMelScale)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import melinv_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _K():
    from pytorch_sound_amd import kernels
    return kernels


@functools.lru_cache(maxsize=None)
def _bank(name):
    from pytorch_sound_amd.utils.mel import mel_filterbank
    if name == 'mel40':
        W = np.load(os.path.join(GOLDEN, 'mel_bands_mel40_in.npz'))['W']
    elif name == 'slaney80':
        W = np.load(os.path.join(GOLDEN, 'mel_bands_slaney80_in.npz'))['W']
    elif name == 'k201':
        W = mel_filterbank(16000, 400, 80)
    elif name == 'hand':
        W = np.array([[1.0, 0.5, 0, 0, 0], [0, 0.5, 1.0, 0.25, 0], [0, 0, 0, 0.75, 0]], dtype=np.float32)      # bin 4 is reached by no filter
    else:
        raise KeyError(name)
    W = np.ascontiguousarray(W, dtype=np.float32)
    W.setflags(write=False)
    return W


def test_the_yardstick_is_a_loop_over_the_frames():
    """solve (numpy expressions over the frame axis) and solve_frame (plain loops, one frame) give the same bits in both dtypes"""
    W = _bank('hand')
    P = R.plan(W, 8)
    Y = R.mels(W, R.spectra(2, 5, 3, seed=1))
    for kind, off in ((R.LOG_NONE, 0.0), (R.LOG_E, 1e-3)):
        Yk = Y if kind == R.LOG_NONE else np.log(Y + 1e-3).astype(np.float32)
        for dt in (np.float64, np.float32):
            x, res = R.solve(P, Yk, 8, kind, off, dtype=dt)
            for n in range(2):
                for f in range(3):
                    xf, rf = R.solve_frame(P, Yk[n, :, f], 8, kind, off, dtype=dt)
                    assert np.array_equal(xf, x[n, :, f]) and rf == res[n, f]


@pytest.mark.parametrize('name', ('hand', 'mel40', 'k201'))
def test_host_equals_the_yardstick(name):
    K = _K()
    W = _bank(name)
    Y = R.mels(W, R.spectra(2, W.shape[1], 5, seed=2))
    P = R.plan(W, 16)
    for n_iter in (0, 1, 16):
        ref, rres = R.solve(P, Y, n_iter)
        got, gres = K.mel_inverse_host(Y, K.mel_inverse_plan(W, 16), n_iter, return_residual=True)
        # the same float64 definition, the sums in another order (a dense product): a few roundings of the largest value
        assert R.rel_err(got, ref) <= 1e-12 and R.rel_err(gres, rres) <= 1e-9
    Yl = np.log(Y.astype(np.float64) + 1e-6)
    ref, _ = R.solve(P, Yl, 4, R.LOG_E, 1e-6, frames=[3, 9])
    got = K.mel_inverse_host(Yl, W, 4, K.LOG_E, 1e-6, frames=[3, 9])
    assert R.rel_err(got, ref) <= 1e-12 and (got[0, :, 3:] == 0).all()


@pytest.mark.parametrize('name', ('hand', 'mel40', 'slaney80', 'k201'))
def test_plan_builder_matches_numpy_to_the_bit(name):
    K = _K()
    assert K.lib().psnd_version() >= 150
    W = _bank(name)
    plan = K.mel_inverse_plan(W, 70)
    raw, host, ref = plan.raw(), plan.host, R.plan(W, 70)
    assert (raw['M'], raw['K'], raw['n_iter_max']) == W.shape + (70,)
    for other in (host, ref):
        assert raw['step'] == other['step'] and raw['L'] == other['L']
        assert np.array_equal(raw['d'], other['d']) and np.array_equal(raw['cinv'], other['cinv'])
        assert np.array_equal(raw['A'], other['A']) and np.array_equal(raw['beta'], other['beta'])
    assert raw['step32'] == float(np.float32(ref['step'])) and np.array_equal(raw['d32'], ref['d'].astype(np.float32))
    assert np.array_equal(raw['cinv32'], ref['cinv'].astype(np.float32))
    live = ref['A'].sum(axis=1) > 0
    assert np.allclose(ref['A'][live].sum(axis=1), 1.0, atol=1e-6)                      # rows sum to 1
    lam = np.linalg.eigvalsh(ref['A'].astype(np.float64) @ ref['A'].astype(np.float64).T).max()
    assert lam <= ref['L'] <= 1.25 * lam                                                # the row-sum bound holds and costs little
    # the band tables walk exactly the non-zero weights, rows and columns
    A = raw['A']
    for bands, vals, mat in ((raw['row_bands'], raw['row_weights'], A), (raw['col_bands'], raw['col_weights'], A.T)):
        total = 0
        for i, (packed, off) in enumerate(bands):
            lo, ln = int(packed) & 0xffff, int(packed) >> 16
            nz = np.flatnonzero(mat[i])
            assert (ln == 0 and nz.size == 0) or (lo == nz[0] and lo + ln == nz[-1] + 1)
            assert np.array_equal(vals[int(off):int(off) + ln], mat[i, lo:lo + ln]) and int(off) == total
            total += ln
        assert total == vals.size
    assert K.mel_inverse_tile(*W.shape) in (2, 4, 8, 16) and K.mel_inverse_tile(128, 2049) >= 1


def test_plan_builder_rejects():
    K = _K()
    lib = K.lib()
    from pytorch_sound_amd import _lib
    W = np.array(_bank('hand'))
    nb = lib.psnd_mel_inverse_plan_bytes(3, 5)
    assert nb > 0
    plan = np.zeros(nb, dtype=np.uint8)
    assert lib.psnd_mel_inverse_plan_build(3, 5, _lib.np_ptr(W), 8, _lib.np_ptr(plan)) == 0
    for bad, word in ((-0.5, '>= 0'), (np.nan, '>= 0'), (np.inf, 'finite')):
        Wb = W.copy()
        Wb[1, 2] = bad
        rc = lib.psnd_mel_inverse_plan_build(3, 5, _lib.np_ptr(Wb), 8, _lib.np_ptr(plan))
        assert rc == _lib.DEFINES['PSND_E_ARG'] and word in lib.psnd_last_error().decode() and '[1, 2]' in lib.psnd_last_error().decode()
        with pytest.raises(K.PsndError, match='>= 0'):
            K.mel_inverse_plan(Wb)
    big = np.zeros((257, 4), dtype=np.float32)
    assert lib.psnd_mel_inverse_plan_bytes(257, 4) == 0 and lib.psnd_mel_inverse_plan_bytes(4, 2050) == 0
    assert lib.psnd_mel_inverse_plan_bytes(256, 2049) > 0
    rc = lib.psnd_mel_inverse_plan_build(257, 4, _lib.np_ptr(big), 8, _lib.np_ptr(plan))
    assert rc == _lib.DEFINES['PSND_E_UNSUPPORTED'] and '256' in lib.psnd_last_error().decode()
    rc = lib.psnd_mel_inverse_plan_build(4, 2050, _lib.np_ptr(big), 8, _lib.np_ptr(plan))
    assert rc == _lib.DEFINES['PSND_E_UNSUPPORTED'] and '2049' in lib.psnd_last_error().decode()
    rc = lib.psnd_mel_inverse_plan_build(3, 5, _lib.np_ptr(W), lib.psnd_mel_inverse_max_iter() + 1, _lib.np_ptr(plan))
    assert rc == _lib.DEFINES['PSND_E_UNSUPPORTED'] and str(lib.psnd_mel_inverse_max_iter()) in lib.psnd_last_error().decode()
    with pytest.raises(K.PsndError, match='256'):
        K.mel_inverse_plan(big).bytes()
    # the launch entry point: argument errors are found before anything touches a device
    rc = lib.psnd_mel_inverse(None, 1, 4, 300, 5, None, 0, 0.0, 1, None, None, None, None)
    assert rc == _lib.DEFINES['PSND_E_UNSUPPORTED'] and '256' in lib.psnd_last_error().decode()
    rc = lib.psnd_mel_inverse(None, 1, 4, 3, 5, None, 7, 0.0, 1, None, None, None, None)
    assert rc == _lib.DEFINES['PSND_E_ARG'] and 'log_kind' in lib.psnd_last_error().decode()
    assert lib.psnd_mel_inverse(None, 1, 4, 3, 5, None, 0, 0.0, 1, None, None, None, None) == _lib.DEFINES['PSND_E_ARG']
    assert lib.psnd_mel_inverse(None, 0, 4, 3, 5, None, 0, 0.0, 1, None, None, None, None) == 0


def test_properties_on_cpu_tensors():
    K = _K()
    W = _bank('mel40')
    X = R.spectra(2, 257, 6, seed=3)
    Y = torch.from_numpy(R.mels(W, X))
    plan = K.mel_inverse_plan(W, 64)
    x, res = K.mel_inverse(Y, plan, 64, return_residual=True)
    assert x.dtype == torch.float32 and x.shape == (2, 257, 6) and res.shape == (2, 6) and not x.requires_grad
    assert bool((x >= 0).all()) and float(res.max()) < 2e-2
    dead = np.flatnonzero(W.sum(axis=0) == 0)
    assert dead.size == 35 and bool((x[:, dead] == 0).all())                            # zero-coverage bins are exactly 0
    x0 = K.mel_inverse(Y.double(), plan, 0)
    h = plan.host
    want0 = h['cinv'][None, :, None] * np.einsum('mk,nmf->nkf', h['A'].astype(np.float64), h['d'][None, :, None] * Y.double().numpy())
    assert x0.dtype == torch.float64 and np.allclose(x0.numpy(), want0, rtol=1e-13, atol=0)        # n_iter = 0 returns x_0
    res8 = K.mel_inverse(Y, plan, 8, return_residual=True)[1]
    assert float(res.max()) < float(res8.max())                                          # more iterations, a smaller residual
    # leading axes, (M, F), frames
    assert torch.equal(K.mel_inverse(Y[:, None], plan, 4)[:, 0], K.mel_inverse(Y, plan, 4))
    assert torch.equal(K.mel_inverse(Y[1], plan, 4), K.mel_inverse(Y, plan, 4)[1])
    dirty = Y.clone()
    dirty[0, :, 2:] = float('nan')
    cut = K.mel_inverse(dirty, plan, 4, frames=[2, 9])
    assert bool((cut[0, :, 2:] == 0).all()) and torch.equal(cut[0, :, :2], K.mel_inverse(Y, plan, 4)[0, :, :2]) and torch.equal(cut[1], K.mel_inverse(Y, plan, 4)[1])
    # a NaN in one frame leaves the others as they were
    bad = Y.clone()
    bad[1, 7, 3] = float('nan')
    a, b = K.mel_inverse(bad.double(), plan, 4), K.mel_inverse(Y.double(), plan, 4)
    keep = torch.ones(2, 6, dtype=torch.bool)
    keep[1, 3] = False
    assert torch.equal(a.permute(0, 2, 1)[keep], b.permute(0, 2, 1)[keep])
    # the three log kinds against exp - offset by hand
    lin = Y.double()
    want = K.mel_inverse(lin, plan, 8)
    for kind, fwd in ((K.LOG_E, torch.log), (K.LOG_10, torch.log10)):
        got = K.mel_inverse(fwd(lin + 1e-3), plan, 8, kind, 1e-3)
        assert R.rel_err(got.numpy(), want.numpy()) < 1e-12
    neg = torch.full((1, 40, 1), -30.0, dtype=torch.float64)                            # exp(-30) - 1e-3 < 0: clamped to b = 0
    z, rz = K.mel_inverse(neg, plan, 8, K.LOG_E, 1e-3, return_residual=True)
    assert bool((z == 0).all()) and float(rz) == 0.0
    # argument errors
    with pytest.raises(K.PsndError, match='bands'):
        K.mel_inverse(Y[:, :39], plan)
    with pytest.raises(K.PsndError, match='built for'):
        K.mel_inverse(Y, plan, 65)
    with pytest.raises(ValueError):
        K.mel_inverse(Y, plan, -1)
    with pytest.raises(ValueError):
        K.mel_inverse(Y, plan, 4, log_kind=9)
    with pytest.raises(K.PsndError):
        K.mel_inverse(Y, plan, 4, frames=[1, 2, 3])
    with pytest.raises(K.PsndError):
        K.mel_inverse(Y.long(), plan, 4)
    for name in ('k17', 'dense24'):                                                       # filterbanks with negative weights: an error, not a clamp
        Wn = np.load(os.path.join(GOLDEN, 'mel_bands_%s_in.npz' % name))['W']
        assert Wn.min() < 0
        with pytest.raises(K.PsndError, match='>= 0'):
            K.mel_inverse(torch.zeros(1, Wn.shape[0], 2), Wn, 1)


def test_empty_band_and_one_filter_per_bin():
    K = _K()
    from pytorch_sound_amd.utils.mel import mel_filterbank
    # a filterbank whose lowest bands are narrower than a bin: at least one filter has no weight at all
    W = mel_filterbank(22050, 64, 17, fmax=2000.0)
    empty = np.flatnonzero(W.sum(axis=1) == 0)
    assert empty.size >= 1 and W.shape == (17, 33)
    X = R.spectra(1, 33, 4, seed=4)
    Y = R.mels(W, X)
    want = K.mel_inverse(torch.from_numpy(Y), W, 8)
    Yd = Y.copy()
    Yd[:, empty] = 123.0                                                                 # whatever the empty band holds is ignored
    assert torch.equal(K.mel_inverse(torch.from_numpy(Yd), W, 8), want) and float(want.max()) > 0
    # one filter per bin, no overlap: exact after 0 iterations, and every later iterate stays there
    Wd = np.zeros((4, 9), dtype=np.float32)
    for m, k in enumerate((1, 3, 4, 7)):
        Wd[m, k] = 0.5 + m
    Xd = np.zeros((1, 9, 3))
    Xd[0, [1, 3, 4, 7]] = np.random.RandomState(0).rand(4, 3) + 0.1
    Yd = np.einsum('mk,nkf->nmf', Wd.astype(np.float64), Xd)
    x0, r0 = K.mel_inverse(torch.from_numpy(Yd), Wd, 0, return_residual=True)
    assert np.allclose(x0.numpy(), Xd, rtol=1e-14, atol=0) and float(r0.max()) < 1e-15
    assert np.allclose(K.mel_inverse(torch.from_numpy(Yd), Wd, 5).numpy(), Xd, rtol=1e-13, atol=0)


def test_public_layers_on_cpu_tensors():
    from pytorch_sound_amd import host as H
    from pytorch_sound_amd.models.sound import MelToWave
    from pytorch_sound_amd.models.transforms import InverseMelScale, LogMelScale, LogMelSpectrogram
    from pytorch_sound_amd.utils import sound as U
    K = _K()
    sr, n_fft, hop, M = 8000, 256, 64, 40
    t = np.arange(4096) / sr
    wav = torch.from_numpy((0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32))[None]
    lm = LogMelSpectrogram(sr, M, n_fft, n_fft, hop)
    mel = lm(wav)
    inv = InverseMelScale(sr, M, n_fft, n_iter=32, log='e')
    assert torch.equal(inv.mel_filter, lm.mel_filter) and 'n_iter=32' in repr(inv)
    mag = inv(mel)
    assert mag.shape == (1, n_fft // 2 + 1, mel.shape[-1]) and bool((mag >= 0).all())
    want = K.mel_inverse(mel, lm.mel_filter, 32, K.LOG_E, 1e-6)
    assert torch.equal(mag, want) and torch.equal(lm.inverse_mel(mel, n_iter=32), want)
    assert torch.equal(U.mel_to_magnitude(mel, lm.mel_filter, 32, 'e'), want)
    assert np.array_equal(U.mel_to_magnitude(mel.numpy(), lm.mel_filter.numpy(), 32, 'e'), want.numpy())
    x, res = inv(mel, return_residual=True)
    assert torch.equal(x, want) and res.shape == (1, mel.shape[-1]) and float(res.max()) < 5e-2
    # forward mel of the inverse reproduces the linear mel
    lin = torch.exp(mel.double()) - 1e-6
    back = torch.matmul(lm.mel_filter.double(), lm.inverse_mel(mel.double()))
    assert float((back - lin).norm() / lin.norm()) < 1e-2
    # the linear and the log10 road
    lin_inv = InverseMelScale(sr, M, n_fft, n_iter=32)
    assert R.rel_err(lin_inv(lin).numpy(), K.mel_inverse(lin, lm.mel_filter, 32).numpy()) == 0.0
    assert R.rel_err(InverseMelScale(sr, M, n_fft, n_iter=32, log='10', log_offset=1e-6)(torch.log10(lin + 1e-6)).numpy(), lin_inv(lin).numpy()) < 1e-9
    with pytest.raises(ValueError):
        InverseMelScale(sr, M, n_fft, log='2')
    with pytest.raises(ValueError):
        InverseMelScale(sr, M, n_fft, n_iter=-1)
    with pytest.raises(RuntimeError):
        inv(mel[:, :-1])
    # mel_to_wave: a 440 Hz tone comes back in its bin
    y = U.mel_to_wave(mel, lm.mel_filter, n_fft, hop, n_iter=32, gl_iter=16, log='e', rand_init=False)
    assert y.shape == (1, (mel.shape[-1] - 1) * hop) and bool(torch.isfinite(y).all())
    inner = y[0].double().numpy()[n_fft:-n_fft]
    peak = int(np.abs(np.fft.rfft(inner * np.hanning(inner.size))).argmax())
    assert round(peak / inner.size * n_fft) == round(440.0 / sr * n_fft) == 14        # the tone's STFT bin (the mel bands there are wider than a bin)
    m2w = MelToWave(sr, M, n_fft, hop, n_iter=32, gl_iter=16, log='e', rand_init=False)
    assert torch.equal(m2w(mel), y) and torch.equal(m2w(mel[0]), y[0]) and m2w(mel, length=1000).shape == (1, 1000)
    assert torch.equal(K.mel_to_wave(mel, lm.mel_filter, lm.stft, 32, 16, 0.99, K.LOG_E, 1e-6, rand_init=False), y)
    # LogMelScale: the reference's module on a magnitude, against host.mel_log
    scale = LogMelScale(sr, M, n_fft, -40.0, -10.0)
    mg = lm.stft.magnitude(wav)
    want = H.mel_log(mg, scale.mel_filter, H.LOG_E, 1e-6, None, np.log(10.0 ** -4), np.log(10.0 ** -1))
    got = scale(mg)
    assert torch.equal(scale.mel_filter, lm.mel_filter) and torch.equal(got, want) and torch.equal(scale(mg[0]), want[0])
    assert float(got.min()) == pytest.approx(np.log(1e-4)) and float(got.max()) == pytest.approx(np.log(0.1))     # both clamps bite
    assert torch.allclose(scale(mg, log_offset=1e-3), H.mel_log(mg, scale.mel_filter, H.LOG_E, 1e-3, None, scale.min_db, scale.max_db))
    with pytest.raises(RuntimeError):
        scale(mg[:, :-1])
    with pytest.raises(ValueError):
        LogMelScale(sr, M, n_fft, 10.0, -60.0)


def test_a_filterbank_is_never_mistaken_for_an_earlier_one():
    """same-shape filterbanks passed one after the other, the earlier one freed each time (the allocator likes to hand its address to the
    next): every answer is that of the filterbank passed.  And a plan keeps the values it was built from."""
    from pytorch_sound_amd.utils import sound as U
    from pytorch_sound_amd.utils.mel import mel_filterbank
    K = _K()
    Y = torch.from_numpy(R.mels(_bank('k201'), R.spectra(1, 201, 3, seed=9)))
    banks = [dict(), dict(fmax=4000.0), dict(fmax=6000.0), dict(fmin=100.0)]
    wants = [K.mel_inverse(Y, K.mel_inverse_plan(mel_filterbank(16000, 400, 80, **kw), 8), 8) for kw in banks]
    assert not torch.equal(wants[0], wants[1])
    for trial in range(6):
        for kw, want in zip(banks, wants):
            for make in (lambda W: torch.from_numpy(W.astype(np.float64)), lambda W: torch.from_numpy(W.copy()), lambda W: W.copy()):
                Wt = make(mel_filterbank(16000, 400, 80, **kw))
                assert torch.equal(U.mel_to_magnitude(Y, Wt, 8), want)
                del Wt
    # a plan does not follow later writes to the array it was built from, before or after its first use
    W = np.array(_bank('k201'))
    plan = K.mel_inverse_plan(W, 8)
    W[:] = mel_filterbank(16000, 400, 80, fmax=4000.0)
    assert torch.equal(K.mel_inverse(Y, plan, 8), wants[0])
    assert np.array_equal(plan.raw()['A'], plan.host['A']) and np.array_equal(plan.raw()['A'], R.plan(_bank('k201'), 8)['A'])
    with pytest.raises(ValueError):
        plan.W[0, 0] = 1.0
