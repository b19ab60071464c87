"""psnd_mel_inverse.hip and kernels.mel_inverse on the GPU against the float64 yardstick tests/melinv_ref.py: frame-tile seams, iteration
counts, six filterbanks, the three log kinds with planted zero and negative bands, ragged items, the residual, frame independence bit for
bit, memory hygiene, layouts and dtypes, the public layers, a side stream, graph capture, no library op.

The comparison rule (the one of tests/test_gpu_griffinlim.py).  EVERY element is compared.  The error of a case is
max |got - ref| / max |ref| against the float64 yardstick on the same float32 inputs.  The bound is 16 times the error of the yardstick's own
float32 variant on the same case (d, cinv, step and every operation rounded to float32, the sums added in float32 in ascending index), with
a floor of one float32 rounding (2^-24): the factor covers the device library's expf / exp10f / sqrtf and the fused multiply-adds of the
kernel's sums.  The bound is computed in the test from the variant and printed; the kernel's own error is printed beside it and never
enters it.  A case is admissible only if its variant error is below 1e-3 (asserted).

Variant errors on the cases of this file (no GPU involved): 3e-8 to 4e-7 at 0 to 8 iterations, up to 6e-6 at 64.

Measured on one MI355X (kernel error / bound).  Frame-tile seams (F = 1, T - 1, T, T + 1, 2 T + 1 with T = 16, 8, 16, 16; N = 1 and 3;
8 iterations): 40 x 257 at most 4.1e-7 / 6.6e-6, 80 x 513 3.6e-7 / 5.6e-6, 80 x 201 2.3e-7 / 3.0e-6, the hand-made 3 x 5 1.9e-7 / 3.0e-6;
the worst ratio is 0.08.  Iterations 0, 1, 2, 8, 64 on 80 x 513: 1.0e-7 / 1.6e-6, 1.5e-7 / 2.2e-6, 1.4e-7 / 1.9e-6, 2.9e-7 / 4.9e-6,
3.2e-6 / 6.2e-5; on 40 x 257 from 1.1e-7 / 1.7e-6 to 2.5e-6 / 4.3e-5, on 80 x 201 from 9.2e-8 / 1.5e-6 to 2.5e-6 / 4.4e-5, on 3 x 5 up to
1.9e-6 / 3.7e-5, on 17 x 33 with its empty bands at most 5.8e-8 / 9.5e-7 (the floor).  128 x 2049 (T = 2, tables read from global
memory) 3.0e-7 / 4.7e-6.  Smooth spectra without peaks, 8 and 64 iterations: at most 4.5e-7 / 5.5e-6 and 3.6e-6 / 4.8e-5.
LOG_E (offsets 1e-6, 1e-3) and LOG_10 with planted zero and negative bands at most 2.4e-7 / 3.8e-6.  Ragged
items over planted NaN / Inf 2.8e-7 / 4.1e-6, the valid part bit-equal to the item run alone.  The residual: at most 4.4e-6 / 1.0e-4 (40 x
257, 64 iterations), worst ratio 0.12 (4.4e-7 / 3.6e-6).  End to end, 64 iterations: slaney80 fixture worst-frame |W x - lin| / |lin|
1.643e-4 on the GPU and 1.643e-4 in float64 on the host; LogMelSpectrogram -> inverse_mel -> forward mel 1.220e-4 and 1.220e-4.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import melinv_ref as R  # noqa: E402
import poison as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ONE_ROUNDING = 2.0 ** -24
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _bank(name):
    from pytorch_sound_amd.utils.mel import mel_filterbank
    if name in ('mel40', 'slaney80'):
        W = np.load(os.path.join(GOLDEN, 'mel_bands_%s_in.npz' % name))['W']
        assert (W.sum(axis=0) == 0).sum() == {'mel40': 35, 'slaney80': 142}[name]
    elif name == 'k201':
        W = mel_filterbank(16000, 400, 80)
        assert W.shape == (80, 201)
    elif name == 'k2049':
        W = mel_filterbank(44100, 4096, 128)
        assert W.shape == (128, 2049)
    elif name == 'hand':
        W = np.array([[1.0, 0.5, 0, 0, 0], [0, 0.5, 1.0, 0.25, 0], [0, 0, 0, 0.75, 0]], dtype=np.float32)
    elif name == 'm17':
        W = mel_filterbank(22050, 64, 17, fmax=2000.0)
        assert W.shape == (17, 33) and (W.sum(axis=1) == 0).sum() >= 1                   # at least one empty band
    else:
        raise KeyError(name)
    W = np.ascontiguousarray(W, dtype=np.float32)
    assert np.isfinite(W).all() and (W >= 0).all()
    W.setflags(write=False)
    return W


@functools.lru_cache(maxsize=None)
def _plans(name, n_iter_max=64):
    """(the library's plan, the yardstick's plan) of a filterbank; built once"""
    return _K().mel_inverse_plan(_bank(name), n_iter_max), R.plan(_bank(name), n_iter_max)


def _tile(name):
    return _K().mel_inverse_tile(*_bank(name).shape)


def _mel(name, N, F, seed, kind=R.LOG_NONE, off=0.0, peaks=True):
    """float32 mels (N, M, F) = W X of non-negative spectra, a smooth envelope with narrow peaks on it or (peaks=False) the envelope alone,
    some bands planted with 0; under a log kind some with a negative linear value"""
    W = _bank(name)
    Y = R.mels(W, R.spectra(N, W.shape[1], F, seed=seed, peaks=peaks))
    rs = np.random.RandomState(500 + seed)
    Y[rs.rand(*Y.shape) < 0.05] = 0.0
    if kind == R.LOG_NONE:
        return Y
    with np.errstate(divide='ignore'):
        L = (np.log(Y.astype(np.float64) + off) if kind == R.LOG_E else np.log10(Y.astype(np.float64) + off)).astype(np.float32)
    L[rs.rand(*Y.shape) < 0.05] = -30.0                  # exp(-30) - off < 0: clamped to 0
    return L


def _check(label, name, Y, n_iter, kind=R.LOG_NONE, off=0.0, frames=None):
    K = _K()
    plan, Pref = _plans(name)
    ref, rres = R.solve(Pref, Y, n_iter, kind, off, frames)
    var, vres = R.solve(Pref, Y, n_iter, kind, off, frames, dtype=np.float32)
    got, gres = K.mel_inverse(_dev(Y), plan, n_iter, kind, off, frames, return_residual=True)
    assert got.dtype == torch.float32 and got.is_cuda and got.shape == ref.shape and gres.shape == rres.shape
    got, gres = got.double().cpu().numpy(), gres.double().cpu().numpy()
    v = R.rel_err(var, ref)
    bound, err = 16.0 * max(v, ONE_ROUNDING), R.rel_err(got, ref)
    rv = R.rel_err(vres, rres)
    rbound, rerr = 16.0 * max(rv, ONE_ROUNDING), R.rel_err(gres, rres)
    print('%s: %s %s n_iter %d kind %d: kernel error %.3g, bound %.3g (variant %.3g); resid: kernel error %.3g, bound %.3g (variant %.3g)'
          % (label, name, Y.shape, n_iter, kind, err, bound, v, rerr, rbound, rv))
    assert v < 1e-3, 'the case is not admissible'
    assert err <= bound, label
    assert (got >= 0).all() and (got[:, _bank(name).sum(axis=0) == 0] == 0).all()        # non-negative; uncovered bins exactly 0
    assert rv < 1e-3 and rerr <= rbound, label
    return got, ref, gres, rres


# ---- against the yardstick --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ('1', 'T-1', 'T', 'T+1', '2T+1'))
@pytest.mark.parametrize('name', ('mel40', 'slaney80', 'k201', 'hand'))
def test_frame_tile_seams(name, which):
    T = _tile(name)
    F = {'1': 1, 'T-1': T - 1, 'T': T, 'T+1': T + 1, '2T+1': 2 * T + 1}[which]
    for N in (1, 3):
        _check('seam %s N=%d' % (which, N), name, _mel(name, N, F, seed=F + N), 8)


@pytest.mark.parametrize('n_iter', (0, 1, 2, 8, 64))
@pytest.mark.parametrize('name', ('mel40', 'slaney80', 'k201', 'hand', 'm17'))
def test_iteration_counts(name, n_iter):
    T = _tile(name)
    _check('n_iter', name, _mel(name, 3, T + 1, seed=n_iter), n_iter)


@pytest.mark.parametrize('n_iter', (8, 64))
@pytest.mark.parametrize('name', ('mel40', 'slaney80', 'k201'))
def test_smooth_spectra(name, n_iter):
    """the envelope alone, no narrow peaks: the inputs on which the loop converges furthest"""
    T = _tile(name)
    _check('smooth', name, _mel(name, 3, T + 1, seed=20 + n_iter, peaks=False), n_iter)


def test_largest_filterbank():
    """K = 2049 bins, M = 128 filters: the smallest frame tile"""
    T = _tile('k2049')
    assert T >= 1 and T * (2 * 2049 + 2 * 128) * 4 <= 65536
    _check('K 2049', 'k2049', _mel('k2049', 1, T + 1, seed=7), 8)


@pytest.mark.parametrize('kind, off', ((R.LOG_E, 1e-6), (R.LOG_E, 1e-3), (R.LOG_10, 1e-6)))
def test_log_kinds(kind, off):
    for name in ('mel40', 'slaney80'):
        T = _tile(name)
        Y = _mel(name, 3, T + 1, seed=31, kind=kind, off=off)
        assert (Y == -30.0).any()
        got, ref, gres, rres = _check('log', name, Y, 8, kind, off)
        # a frame whose every band is clamped: b = 0, x = 0, resid = 0
        Z = np.full_like(Y, -30.0)
        x, res = _K().mel_inverse(_dev(Z), _plans(name)[0], 8, kind, off, return_residual=True)
        assert bool((x == 0).all()) and bool((res == 0).all())


def test_ragged_items_over_planted_nans():
    K = _K()
    name = 'mel40'
    T = _tile(name)
    F = 2 * T + 3
    frames = [0, 1, F, F + 9, -2, T + 1]
    clean = _mel(name, len(frames), F, seed=41)
    dirty = clean.copy()
    for n, fn in enumerate(frames):
        dirty[n, :, min(max(fn, 0), F):] = np.nan if n % 2 == 0 else np.inf
    got, ref, gres, _ = _check('ragged', name, dirty, 8, frames=frames)
    assert np.isfinite(got).all() and np.isfinite(gres).all()
    plan = _plans(name)[0]
    for n, fn in enumerate(frames):
        fn = min(max(fn, 0), F)
        assert (got[n, :, fn:] == 0).all() and (gres[n, fn:] == 0).all()
        if fn:
            alone = K.mel_inverse(_dev(clean[n:n + 1, :, :fn]), plan, 8).double().cpu().numpy()
            assert np.array_equal(alone[0], got[n, :, :fn]), n
    a = K.mel_inverse(_dev(dirty), plan, 8, frames=torch.tensor(frames, device=DEV))
    b = K.mel_inverse(_dev(dirty), plan, 8, frames=torch.tensor(frames, dtype=torch.int32))
    assert np.array_equal(a.double().cpu().numpy(), got) and P.same_bits(a, b)


def test_same_bits_on_poisoned_memory():
    """the outputs come from torch.empty: every slot, the zeros behind an item's frames and the residual included, is written by the call"""
    K = _K()
    name = 'mel40'
    T = _tile(name)
    F = 2 * T + 3
    frames = torch.tensor([0, 1, F, T + 1], device=DEV)
    Y = _mel(name, 4, F, seed=43)
    Y[0], Y[1, :, 1:], Y[3, :, T + 1:] = np.nan, np.nan, np.nan
    d, plan = _dev(Y), _plans(name)[0]
    first = P.assert_same_bits(lambda: list(K.mel_inverse(d, plan, 4, frames=frames, return_residual=True)))
    assert (first[0][0] == 0).all() and first[0][2].abs().max() > 0.01 and (first[1][0] == 0).all()


# ---- frame independence, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('slaney80', 'k201'))
def test_a_frame_depends_on_its_own_column_alone(name):
    K = _K()
    plan = _plans(name)[0]
    T = _tile(name)
    F = 2 * T + 3
    base = _mel(name, 3, F, seed=51)
    col = base[0, :, 0].copy()
    alone, ralone = K.mel_inverse(_dev(col[None, :, None]), plan, 16, return_residual=True)
    places = ((0, 0), (0, T - 1), (1, T), (2, 2 * T + 2), (1, 5))
    for seed in (52, 53):                                # other neighbours each time
        Y = _mel(name, 3, F, seed=seed)
        for n, f in places:
            Y[n, :, f] = col
        x, res = K.mel_inverse(_dev(Y), plan, 16, return_residual=True)
        for n, f in places:
            assert P.same_bits(x[n, :, f], alone[0, :, 0]) and P.same_bits(res[n, f], ralone[0, 0]), (n, f)
    # a frame with a planted NaN or Inf leaves every other frame's bits as they are
    Y = _mel(name, 3, F, seed=54)
    want, rwant = K.mel_inverse(_dev(Y), plan, 16, return_residual=True)
    for value in (np.nan, np.inf, -np.inf):
        bad = Y.copy()
        bad[1, 3, T] = value
        bad[2, :, 1] = value
        x, res = K.mel_inverse(_dev(bad), plan, 16, return_residual=True)
        keep = torch.ones(3, F, dtype=torch.bool, device=DEV)
        keep[1, T] = keep[2, 1] = False
        assert P.same_bits(x.permute(0, 2, 1)[keep], want.permute(0, 2, 1)[keep]) and P.same_bits(res[keep], rwant[keep])
    again = K.mel_inverse(_dev(Y), plan, 16)
    assert P.same_bits(again, want)                      # repeated launches agree bit for bit


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _worst_frame(W, x, lin):
    """max over the frames of |W x - lin| / |lin| in float64; a frame with lin = 0 (the fixture has one) must come out as x = 0 and is left out"""
    x = np.asarray(x, np.float64)
    r = np.einsum('mk,nkf->nmf', W.astype(np.float64), x) - lin
    top = np.linalg.norm(lin, axis=1)
    assert (x.transpose(0, 2, 1)[top == 0] == 0).all()
    return float((np.linalg.norm(r, axis=1)[top > 0] / top[top > 0]).max())


def test_slaney80_fixture_end_to_end():
    """the linear mels of the fixture, 64 iterations: the GPU result explains the mel as well as the float64 host result does"""
    K = _K()
    z = np.load(os.path.join(GOLDEN, 'mel_bands_slaney80_in.npz'))
    W, lin = _bank('slaney80'), np.maximum(z['lin'].astype(np.float32), 0.0)
    plan = _plans('slaney80')[0]
    host = K.mel_inverse_host(lin, plan, 64)
    got = K.mel_inverse(_dev(lin), plan, 64).double().cpu().numpy()
    lin64 = lin.astype(np.float64)
    h, g = _worst_frame(W, host, lin64), _worst_frame(W, got, lin64)
    print('slaney80 fixture %s, 64 iterations: worst-frame residual GPU %.4g, float64 host %.4g' % (lin.shape, g, h))
    assert g <= 2.0 * h + 16.0 * ONE_ROUNDING


def test_logmel_inverse_mel_forward_mel_chain():
    from pytorch_sound_amd.models.transforms import LogMelSpectrogram
    K = _K()
    sr, n_fft, hop, M = 22050, 1024, 256, 80
    rs = np.random.RandomState(61)
    t = np.arange(8192) / sr
    wav = (0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 1300.0 * t + 1.0) + 0.02 * rs.randn(t.size)).astype(np.float32)
    lm = LogMelSpectrogram(sr, M, n_fft, n_fft, hop).to(DEV)
    mel = lm(torch.from_numpy(wav)[None].to(DEV))
    mag = lm.inverse_mel(mel, n_iter=64)
    assert mag.shape == (1, n_fft // 2 + 1, mel.shape[-1]) and mag.is_cuda and bool((mag >= 0).all())
    W = lm.mel_filter.cpu().numpy()
    lin = np.maximum(np.exp(mel.double().cpu().numpy()) - 1e-6, 0.0)
    host = K.mel_inverse(mel.cpu().double(), W, 64, K.LOG_E, 1e-6).numpy()          # the CPU path in float64 on the same mel
    h, g = _worst_frame(W, host, lin), _worst_frame(W, mag.double().cpu().numpy(), lin)
    print('LogMelSpectrogram -> inverse_mel -> forward mel: worst-frame residual GPU %.4g, float64 host %.4g' % (g, h))
    assert g <= 2.0 * h + 16.0 * ONE_ROUNDING and h < 0.1


def test_mel_to_wave_brings_a_tone_back():
    from pytorch_sound_amd.models.sound import MelToWave
    from pytorch_sound_amd.models.transforms import LogMelSpectrogram
    from pytorch_sound_amd.utils import sound as U
    sr, n_fft, hop, M = 8000, 256, 64, 40
    wav = torch.from_numpy((0.5 * np.sin(2 * np.pi * 440.0 * np.arange(8192) / sr)).astype(np.float32))[None].to(DEV)
    lm = LogMelSpectrogram(sr, M, n_fft, n_fft, hop).to(DEV)
    mel = lm(wav)
    y = U.mel_to_wave(mel, lm.mel_filter, n_fft, hop, n_iter=32, gl_iter=16, log='e', rand_init=False)
    assert y.is_cuda and y.shape == (1, (mel.shape[-1] - 1) * hop) and bool(torch.isfinite(y).all())
    inner = y[0].double().cpu().numpy()[n_fft:-n_fft]
    peak = int(np.abs(np.fft.rfft(inner * np.hanning(inner.size))).argmax())
    assert round(peak / inner.size * n_fft) == round(440.0 / sr * n_fft)                 # the tone's STFT bin
    assert float(y[0, n_fft:-n_fft].abs().max()) > 0.1
    m = MelToWave(sr, M, n_fft, hop, n_iter=32, gl_iter=16, log='e', rand_init=False).to(DEV)
    assert P.same_bits(m(mel), y) and P.same_bits(m(mel[0]), y[0])
    assert U.mel_to_wave(mel, lm.mel_filter, n_fft, hop, n_iter=4, gl_iter=2, log='e').shape == y.shape      # the random start


# ---- hygiene ----------------------------------------------------------------------------------------------------------------------------
def test_memory_around_the_outputs_and_odd_alignment():
    """the entry point itself on buffers that start 4 bytes past a 16-byte boundary, with guard words around the outputs"""
    K = _K()
    name = 'k201'
    W = _bank(name)
    M, Kb = W.shape
    T = _tile(name)
    N, F = 3, 2 * T + 1
    Y = _dev(_mel(name, N, F, seed=71))
    plan = _plans(name)[0]
    want, rwant = K.mel_inverse(Y, plan, 8, return_residual=True)
    GUARD = 64
    big_y = torch.zeros(N * M * F + 1, device=DEV)
    y_off = big_y[1:].reshape(N, M, F)
    y_off.copy_(Y)
    big_o = torch.full((N * Kb * F + 2 * GUARD + 1,), -7.0, device=DEV)
    big_r = torch.full((N * F + 2 * GUARD + 1,), -7.0, device=DEV)
    o = big_o[GUARD + 1:GUARD + 1 + N * Kb * F].reshape(N, Kb, F)
    r = big_r[GUARD + 1:GUARD + 1 + N * F].reshape(N, F)
    assert y_off.data_ptr() % 16 == 4 and o.data_ptr() % 16 == 4 and r.data_ptr() % 16 == 4
    with K.on(Y.device) as hip:
        hip.psnd_mel_inverse(y_off, N, F, M, Kb, plan.tensor(Y.device), K.LOG_NONE, 0.0, 8, None, o, r)
    torch.cuda.synchronize()
    assert P.same_bits(o, want) and P.same_bits(r, rwant)
    for big, size in ((big_o, N * Kb * F), (big_r, N * F)):
        assert bool((big[:GUARD + 1] == -7.0).all()) and bool((big[GUARD + 1 + size:] == -7.0).all())
    assert P.same_bits(K.mel_inverse(y_off, plan, 8), want)
    # more iterations than the plan has momentum factors for: the wrapper raises, the entry point fills its outputs with NaN
    with pytest.raises(K.PsndError, match='built for'):
        K.mel_inverse(Y, plan, plan.n_iter_max + 1)
    with K.on(Y.device) as hip:
        hip.psnd_mel_inverse(y_off, N, F, M, Kb, plan.tensor(Y.device), K.LOG_NONE, 0.0, plan.n_iter_max + 1, None, o, r)
    torch.cuda.synchronize()
    assert bool(torch.isnan(o).all()) and bool(torch.isnan(r).all()) and bool((big_o[:GUARD + 1] == -7.0).all())
    # a plan built for another (M, K), and memory that is no plan at all: the same loud answer, nothing around the outputs touched
    other = _plans('mel40')[0].tensor(Y.device)
    for table in (other, torch.zeros(4096, dtype=torch.uint8, device=DEV)):
        o.fill_(1.0), r.fill_(1.0)
        with K.on(Y.device) as hip:
            hip.psnd_mel_inverse(y_off, N, F, M, Kb, table, K.LOG_NONE, 0.0, 8, None, o, r)
        torch.cuda.synchronize()
        assert bool(torch.isnan(o).all()) and bool(torch.isnan(r).all())
        for big, size in ((big_o, N * Kb * F), (big_r, N * F)):
            assert bool((big[:GUARD + 1] == -7.0).all()) and bool((big[GUARD + 1 + size:] == -7.0).all())


def test_layouts_dtypes_and_errors():
    K = _K()
    name = 'mel40'
    W = _bank(name)
    T = _tile(name)
    N, F = 2, T + 3
    Y = _dev(_mel(name, N, F, seed=81))
    plan = _plans(name)[0]
    want = K.mel_inverse(Y, plan, 8)
    lead = K.mel_inverse(Y.reshape(N, 1, 40, F), plan, 8)
    assert lead.shape == (N, 1, 257, F) and P.same_bits(lead[:, 0], want)
    assert P.same_bits(K.mel_inverse(Y[0], plan, 8), want[0])
    s = torch.empty(F, 40, N, device=DEV)
    s.copy_(Y.permute(2, 1, 0))
    view = s.permute(2, 1, 0)
    assert not view.is_contiguous() and torch.equal(view, Y)
    assert P.same_bits(K.mel_inverse(view, plan, 8), want)
    assert P.same_bits(K.mel_inverse(Y, W, 8), want) and P.same_bits(K.mel_inverse(Y, torch.from_numpy(np.array(W)).to(DEV), 8), want)
    for dt in (torch.float16, torch.bfloat16):
        h = Y.to(dt)
        a, b = K.mel_inverse(h, plan, 8, return_residual=True), K.mel_inverse(h.float(), plan, 8, return_residual=True)
        assert a[0].dtype == dt and P.same_bits(a[0], b[0].to(dt)) and a[1].dtype == torch.float32 and P.same_bits(a[1], b[1])
    with pytest.raises(K.PsndError, match='float64'):
        K.mel_inverse(Y.double(), plan, 8)
    with pytest.raises(K.PsndError):
        K.mel_inverse(Y.int(), plan, 8)
    with pytest.raises(K.PsndError, match='bands'):
        K.mel_inverse(Y[:, :39], plan, 8)
    Wn = np.load(os.path.join(GOLDEN, 'mel_bands_k17_in.npz'))['W']                   # negative weights: an error, not a clamp
    assert Wn.min() < 0
    with pytest.raises(K.PsndError, match='>= 0'):
        K.mel_inverse(torch.zeros(1, Wn.shape[0], 4, device=DEV), Wn, 8)
    e = torch.zeros(2, 40, 0, device=DEV)
    assert K.mel_inverse(e, plan, 8).shape == (2, 257, 0)
    assert not K.mel_inverse(Y.clone().requires_grad_(True), plan, 8).requires_grad


def test_public_layers_side_stream_and_graph_capture():
    from pytorch_sound_amd.models.sound import MelToWave
    from pytorch_sound_amd.models.transforms import InverseMelScale, LogMelScale, LogMelSpectrogram
    from pytorch_sound_amd.utils import sound as U
    from pytorch_sound_amd import host as H
    K = _K()
    sr, n_fft, hop, M = 8000, 256, 64, 40
    rs = np.random.RandomState(91)
    wavs = torch.from_numpy((0.3 * rs.randn(2, 4096)).astype(np.float32)).to(DEV)
    lm = LogMelSpectrogram(sr, M, n_fft, n_fft, hop).to(DEV)
    mel, other = lm(wavs), lm(0.5 * wavs.flip(1))
    inv = InverseMelScale(sr, M, n_fft, n_iter=16, log='e').to(DEV)
    want = K.mel_inverse(mel, lm.mel_filter, 16, K.LOG_E, 1e-6)
    assert P.same_bits(inv(mel), want) and P.same_bits(lm.inverse_mel(mel, n_iter=16), want)
    assert P.same_bits(U.mel_to_magnitude(mel, lm.mel_filter, 16, 'e'), want)
    x, res = inv(mel, return_residual=True)
    assert P.same_bits(x, want) and res.shape == (2, mel.shape[-1]) and bool(torch.isfinite(res).all())
    # LogMelScale on the GPU against the host formula in float64
    scale = LogMelScale(sr, M, n_fft, -40.0, -10.0).to(DEV)
    mg = lm.stft.magnitude(wavs)
    ref = H.mel_log(mg.double().cpu(), scale.mel_filter.double().cpu(), H.LOG_E, 1e-6, None, scale.min_db, scale.max_db)
    got = scale(mg)
    assert got.is_cuda and got.shape == ref.shape and float((got.double().cpu() - ref).abs().max()) < 1e-4
    assert P.same_bits(scale(mg[0]), got[0])
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = inv(mel)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert P.same_bits(on_side, want)
    # capture of mel_inverse: after the calls above nothing is copied from the host
    want_other = inv(other)
    buf = mel.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = inv(buf)
    graph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(out, want)
    buf.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(out, want_other) and not P.same_bits(want_other, want)
    # ... and of MelToWave with a zero first phase
    m = MelToWave(sr, M, n_fft, hop, n_iter=16, gl_iter=4, log='e', rand_init=False).to(DEV)
    eager, eager_other = m(mel), m(other)
    buf.copy_(mel)
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        wave = m(buf)
    g2.replay()
    torch.cuda.synchronize()
    assert P.same_bits(wave, eager)
    buf.copy_(other)
    g2.replay()
    torch.cuda.synchronize()
    assert P.same_bits(wave, eager_other) and not P.same_bits(eager_other, eager)


FORBIDDEN = ('aten.bmm', 'aten.baddbmm', 'aten.mm.', 'aten.addmm', 'aten.matmul', 'aten.einsum', 'aten.linalg', 'aten.convolution', 'aten.miopen',
             'aten.clamp', 'aten.relu', 'aten.maximum', 'aten.exp', 'aten.pow', 'aten.sub', 'aten.add.', 'aten.mul', 'aten.div', 'aten.sqrt',
             'aten.sum', 'aten._fft')


class _Forbid(TorchDispatchMode):
    """the dispatch mode of tests/test_gpu_no_library_paths.py, declared again here, with the ops a loop in library ops would take"""

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if any(name.startswith(f) for f in FORBIDDEN):
            flat = torch.utils._pytree.tree_leaves((args, kwargs or {}))
            if any(isinstance(a, torch.Tensor) and a.is_cuda for a in flat):
                raise AssertionError('library op %s reached with a HIP tensor' % name)
        return func(*args, **(kwargs or {}))


def test_no_library_op_is_reached():
    K = _K()
    name = 'slaney80'
    plan = _plans(name)[0]
    T = _tile(name)
    Y = _dev(_mel(name, 2, T + 1, seed=95, kind=R.LOG_E, off=1e-6))
    fr = torch.tensor([T, 3], device=DEV)
    want = K.mel_inverse(Y, plan, 8, K.LOG_E, 1e-6, fr, return_residual=True)
    with _Forbid():
        got = K.mel_inverse(Y, plan, 8, K.LOG_E, 1e-6, fr, return_residual=True)
    assert P.same_bits(got[0], want[0]) and P.same_bits(got[1], want[1])
    with pytest.raises(AssertionError, match='library op'):
        with _Forbid():
            torch.matmul(torch.from_numpy(np.array(_bank(name))).to(DEV), want[0])
