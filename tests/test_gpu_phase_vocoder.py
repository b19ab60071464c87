"""psnd_phase_vocoder.hip on the GPU against the float64 loop yardstick tests/pv_ref.py: pass and carry seams, the rates, edge sizes, zeros,
error growth on long rows, known answers, ragged rows, non-finite input, layouts and dtypes, memory hygiene, determinism, streams and graph
capture, and the public functions (utils.sound.time_stretch / pitch_shift, models.sound.TimeStretch / PitchShift).

The comparison rule.  EVERY element is compared.  The function is continuous in its inputs apart from floor, which both sides take of the
same double product.  The error of a case is max |Y - Y_ref| / max |Y_ref| over both parts, against the float64 yardstick on the same
float32 inputs.  The bound is 16 times the error of the yardstick's own float32 variant on the same case (float32 arctan2, hypot,
interpolation and polar step; the angle differences summed in float64 and reduced modulo a turn), with a floor of one float32 rounding
(2^-24) for the tiny cases: the variant is the kernel's arithmetic with numpy's correctly rounded elementary functions, the factor covers
the device library's atan2f / sincosf (a few ulp) and the other order of accumulation - the factor tests/test_gpu_pitch.py uses for the
same reason.  The bound is computed in the test from the variant and printed; the kernel's own error is printed beside it and never
enters it.  Variant errors on the cases of this file (no GPU involved): 6e-8 to 9e-7 for up to 450 output frames, 2.1e-6 on the long rows
(3226 frames), 1.5e-5 where one input pair serves 333 outputs.  test_error_growth also prints what the variant shows with its phase
summed as a plain float32 number: 2.1e-5 on these rows, ten times the variant (in the header's wording the raw differences nearly
telescope, so the sum stays within a few hundred radians; the textbook's unwrapped sum in float32 is what drifts to 2e-3).

Measured on one MI355X (kernel error / bound): seams at most 1.3e-6 / 2.6e-5; the rates 1 ... 3.7 and 40 between 1.5e-7 / 2.5e-6 and
8.9e-7 / 1.6e-5; rate 0.03 1.1e-5 / 1.8e-4; rate 0.003 1.1e-4 / 5.7e-4 (the worst ratio, 0.20: one pair's angle
error is added 333 times there, on both sides); F of 1 and 2 at most 9.9e-7 / 6.7e-6; zeros 2.1e-6 / 2.9e-5; the long rows 3.3e-6 / 3.4e-5; the identity
1.7e-7 / 2.7e-6 (against X itself the same); closed form against the formula at most 9.4e-7 / 1.8e-5; ragged 4.6e-7 / 7.4e-6;
non-finite rows 1.4e-6 / 1.5e-5."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pv_ref as R  # noqa: E402
import poison as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ONE_ROUNDING = 2.0 ** -24


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pass():
    return _K().pv_pass()                               # read from the library, not mirrored (psnd_pv_pass of include/psnd.h)


def _run(re, im, rate, shape, frames=None):
    """re, im: (rows, F) float32 with rows = N K for shape = (N, K) -> the kernel's (yre, yim) as (rows, J) numpy arrays"""
    N, Kb = shape
    out = _K().phase_vocoder(_dev(re).reshape(N, Kb, -1), _dev(im).reshape(N, Kb, -1), rate, frames)
    assert out[0].dtype == torch.float32 and out[0].is_cuda and out[0].shape[:2] == (N, Kb)
    return tuple(o.reshape(N * Kb, -1).cpu().numpy() for o in out)


_REFS = {}


def _refs(key, re, im, rate, fr_rows=None):
    """(float64 yardstick, its float32 variant) of a case, computed once per key and left unchanged"""
    if key not in _REFS:
        ref, var = R.pv(re, im, rate, fr_rows), R.pv(re, im, rate, fr_rows, dtype=np.float32)
        for a in ref + var:
            a.setflags(write=False)
        _REFS[key] = (ref, var)
    return _REFS[key]


def _check(label, re, im, rate, shape, frames=None):
    fr_rows = None if frames is None else np.repeat(np.asarray(frames), shape[1])
    ref, var = _refs(label, re, im, rate, fr_rows)
    got = _run(re, im, rate, shape, frames)
    bound = 16.0 * max(R.rel_err(var, ref), ONE_ROUNDING)
    err = R.rel_err(got, ref)
    print('%s: %d rows x %d -> %d frames, rate %g: kernel error %.3g, bound %.3g (variant %.3g)'
          % (label, re.shape[0], re.shape[1], ref[0].shape[1], rate, err, bound, bound / 16.0))
    assert got[0].shape == ref[0].shape
    assert err <= bound, label
    return got, ref


def _frames_for(J, rate):
    """an input length F with pv_frames(F, rate) == J"""
    for F in range(0, int(J * rate) + 4):
        if R.frames(F, rate) == J:
            return F
    raise AssertionError('no F gives %d frames at rate %g' % (J, rate))


# ---- seams ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ('1', 'P-1', 'P', 'P+1', '2P+1'))
def test_pass_and_carry_seams(which):
    """J around the frames of a wave pass; 1 and 3 rows, and N = 2 with K = 5: the row -> (n, k) mapping and a row count that is no multiple
    of the waves of a workgroup.  (The kernel does not split rows: there is no other seam.)"""
    Pn = _pass()
    J = {'1': 1, 'P-1': Pn - 1, 'P': Pn, 'P+1': Pn + 1, '2P+1': 2 * Pn + 1}[which]
    for rate in (1.0, 1.25):
        F = _frames_for(J, rate)
        for shape in ((1, 1), (1, 3), (2, 5)):
            re, im = R.seeded_spectrum(shape[0], shape[1], F, seed=J + shape[1])
            got, ref = _check('seam J=%s rate=%g rows=%s' % (which, rate, shape), re, im, rate, shape)
            assert got[0].shape[1] == J


@pytest.mark.parametrize('rate', (1.0, 0.5, 2.0, 0.8, 1.25, 1.0 / 3.0, 3.7, 0.03, 40.0, 0.003))
def test_rates(rate):
    """0.03: one input pair serves 33 consecutive outputs, 0.003: more than a whole pass of them; 40: a few frames out"""
    F = {0.03: 12, 0.003: 3}.get(rate, 150)
    re, im = R.seeded_spectrum(2, 5, F, seed=17)
    got, ref = _check('rate %g' % rate, re, im, rate, (2, 5))
    assert got[0].shape[1] == _K().pv_frames(F, rate) == R.frames(F, rate)


def test_edge_sizes():
    K = _K()
    for F in (1, 2):
        for rate in (0.5, 1.0, 2.0, 0.1):
            re, im = R.seeded_spectrum(1, 3, F, seed=F)
            _check('F=%d rate=%g' % (F, rate), re, im, rate, (1, 3))
    e = torch.zeros(2, 3, 0, device=DEV)
    out = K.phase_vocoder(e, e, 0.5)
    assert out[0].shape == (2, 3, 0) and out[1].shape == (2, 3, 0)
    e = torch.zeros(0, 3, 9, device=DEV)
    assert K.phase_vocoder(e, e, 0.5)[0].shape == (0, 3, 18)


def test_zeros():
    """arg 0 = 0 whatever the signs of the zeros; an all-zero row gives exact zeros"""
    re, im = R.seeded_spectrum(1, 4, 300, seed=5)
    re[1, 40:90] = im[1, 40:90] = 0.0
    re[1, 50:60], im[1, 55:70] = -0.0, -0.0
    re[1, 200] = im[1, 200] = 0.0
    im[2, 100:140] = 0.0                                 # real, both signs: angles 0 and pi
    re[3] = im[3] = 0.0
    re[3, 7], im[3, 9] = -0.0, -0.0
    for rate in (0.8, 1.25):
        got, ref = _check('zeros rate=%g' % rate, re, im, rate, (1, 4))
        assert (got[0][3] == 0).all() and (got[1][3] == 0).all()
        assert np.abs(got[0][1]).max() > 0.1


def test_error_growth_on_long_rows():
    """3 rows x 3000 frames at rate 0.93.  The bound comes from the variant that sums its phase in float64; what the same variant shows
    with a plain float32 phase is printed beside it."""
    re, im = R.seeded_spectrum(1, 3, 3000, seed=9)
    got, ref = _check('long rows', re, im, 0.93, (1, 3))
    naive = R.rel_err(R.pv(re, im, 0.93, dtype=np.float32, phase32=True), ref)
    bound = 16.0 * R.rel_err(_REFS['long rows'][1], ref)
    print('long rows: a plain float32 phase would show %.3g against the bound %.3g' % (naive, bound))
    assert got[0].shape[1] == R.frames(3000, 0.93) == 3226


def test_rate_one_is_the_identity():
    re, im = R.seeded_spectrum(2, 5, 300, seed=3)
    got, ref = _check('identity', re, im, 1.0, (2, 5))
    var = _REFS['identity'][1]
    bound = 16.0 * max(R.rel_err(var, (re, im)), ONE_ROUNDING)
    err = R.rel_err(got, (re, im))
    print('identity: Y against X %.3g, bound %.3g' % (err, bound))
    assert err <= bound


@pytest.mark.parametrize('rate', (0.5, 0.75, 1.0 / 3.0, 1.3, 1.5, 2.0))
def test_rotating_rows_in_closed_form(rate):
    rs = np.random.RandomState(7)
    rows, F, n, hop = 6, 120, 1024, 256
    A, theta, nu = rs.uniform(0.1, 3.0, (rows, 1)), rs.uniform(-np.pi, np.pi, (rows, 1)), rs.uniform(0.0, 512.0, (rows, 1))
    X = A * np.exp(1j * (theta + 2.0 * np.pi * nu * hop * np.arange(F) / n))
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    got, ref = _check('closed form rate=%g' % rate, re, im, rate, (2, 3))
    j = np.arange(ref[0].shape[1])
    inner = np.floor(j * rate).astype(int) + 1 < F
    want = A * np.exp(1j * (theta + 2.0 * np.pi * nu * hop * j / n))
    want = (want.real[:, inner], want.imag[:, inner])
    var = _REFS['closed form rate=%g' % rate][1]
    bound = 16.0 * max(R.rel_err((var[0][:, inner], var[1][:, inner]), want), ONE_ROUNDING)
    err = R.rel_err((got[0][:, inner], got[1][:, inner]), want)
    print('closed form rate=%g: kernel against the formula %.3g, bound %.3g' % (rate, err, bound))
    assert err <= bound


# ---- ragged rows, non-finite input ----------------------------------------------------------------------------------------------------------
def _ragged(F=70, Kb=3):
    frames = [0, 1, F, F + 9, -2, 33]
    re, im = R.seeded_spectrum(len(frames), Kb, F, seed=21)
    dirty_re, dirty_im = re.copy(), im.copy()
    for n, fn in enumerate(frames):                     # what lies behind a row's length must not be read: NaNs there
        fn = min(max(fn, 0), F)
        dirty_re[n * Kb:(n + 1) * Kb, fn:] = np.nan
        dirty_im[n * Kb:(n + 1) * Kb, fn:] = np.inf
    return frames, re, im, dirty_re, dirty_im


@pytest.mark.parametrize('rate', (0.8, 1.25))
def test_ragged_frames(rate):
    K = _K()
    F, Kb = 70, 3
    frames, re, im, dre, dim = _ragged(F, Kb)
    got, ref = _check('ragged rate=%g' % rate, dre, dim, rate, (len(frames), Kb), frames)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    for n, fn in enumerate(frames):
        fn = min(max(fn, 0), F)
        Jn = R.frames(fn, rate)
        rows = slice(n * Kb, (n + 1) * Kb)
        assert (got[0][rows, Jn:] == 0).all() and (got[1][rows, Jn:] == 0).all(), n
        if fn:
            alone = _run(re[rows, :fn], im[rows, :fn], rate, (1, Kb))
            assert alone[0].shape[1] == Jn
            assert np.array_equal(alone[0], got[0][rows, :Jn]) and np.array_equal(alone[1], got[1][rows, :Jn]), n
    # frames as a device tensor, and as a tensor of another integer type
    a = K.phase_vocoder(_dev(dre).reshape(-1, Kb, F), _dev(dim).reshape(-1, Kb, F), rate, torch.tensor(frames, device=DEV))
    b = K.phase_vocoder(_dev(dre).reshape(-1, Kb, F), _dev(dim).reshape(-1, Kb, F), rate, torch.tensor(frames, dtype=torch.int32))
    assert np.array_equal(a[0].reshape(-1, a[0].shape[-1]).cpu().numpy(), got[0]) and P.same_bits(a[1], b[1])


@pytest.mark.parametrize('rate', (0.8, 1.0, 2.5))
def test_non_finite_input_is_nan_from_there_on_in_its_row_alone(rate):
    re, im = R.seeded_spectrum(2, 4, 400, seed=31)
    clean = _run(re, im, rate, (2, 4))
    bre, bim = re.copy(), im.copy()
    bre[5, 150], bim[5, 333] = np.nan, -np.inf
    bim[2, 0] = np.inf                                  # lost from the first frame on
    got, ref = _check('non-finite rate=%g' % rate, bre, bim, rate, (2, 4))
    J = got[0].shape[1]
    i = np.floor(np.arange(J) * rate).astype(int)
    reads = (i == 150) | (i + 1 == 150)
    assert reads.any()                                  # at rate 2.5 frame 150 is read as an i_j: 60 * 2.5
    first = int(np.flatnonzero(reads)[0])
    for y, c in zip(got, clean):
        assert np.isnan(y[5, first:]).all() and np.isfinite(y[5, :first]).all() and first > 10
        assert np.isnan(y[2]).all()
        for r in (0, 1, 3, 4, 6, 7):
            assert np.array_equal(y[r], c[r]), r
        assert np.array_equal(y[5, :first], c[5, :first])


def test_an_element_no_frame_reads_changes_nothing():
    re, im = R.seeded_spectrum(1, 2, 200, seed=33)
    clean = _run(re, im, 3.7, (1, 2))
    i = np.floor(np.arange(clean[0].shape[1]) * 3.7).astype(int)
    skipped = sorted(set(range(200)) - set(i) - set(i + 1))
    bre = re.copy()
    bre[1, skipped] = np.nan
    got = _run(bre, im, 3.7, (1, 2))
    assert len(skipped) > 50 and np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])


# ---- layouts, dtypes, memory, streams -------------------------------------------------------------------------------------------------------
def test_layouts_and_dtypes():
    K = _K()
    re, im = R.seeded_spectrum(2, 5, 130, seed=41)
    a, b = _dev(re).reshape(2, 5, 130), _dev(im).reshape(2, 5, 130)
    want = K.phase_vocoder(a, b, 0.8)
    lead = K.phase_vocoder(a.reshape(2, 1, 5, 130), b.reshape(2, 1, 5, 130), 0.8)
    assert lead[0].shape == (2, 1, 5, 163) and P.same_bits(lead[0][:, 0], want[0]) and P.same_bits(lead[1][:, 0], want[1])
    two = K.phase_vocoder(a[0], b[0], 0.8)              # (K, F): one item
    assert two[0].shape == (5, 163) and P.same_bits(two[0], want[0][0])
    ta, tb = torch.empty(130, 5, 2, device=DEV), torch.empty(130, 5, 2, device=DEV)
    ta.copy_(a.permute(2, 1, 0)), tb.copy_(b.permute(2, 1, 0))
    va, vb = ta.permute(2, 1, 0), tb.permute(2, 1, 0)
    assert not va.is_contiguous() and torch.equal(va, a)
    got = K.phase_vocoder(va, vb, 0.8)
    assert P.same_bits(got[0], want[0]) and P.same_bits(got[1], want[1])
    big = torch.zeros(2 * 5 * 130 + 1, device=DEV)
    off = big[1:].reshape(2, 5, 130)
    off.copy_(a)
    assert off.data_ptr() % 16 == 4
    assert P.same_bits(K.phase_vocoder(off, b, 0.8)[0], want[0])
    for dt in (torch.float16, torch.bfloat16):
        ha, hb = a.to(dt), b.to(dt)
        h, f = K.phase_vocoder(ha, hb, 0.8), K.phase_vocoder(ha.float(), hb.float(), 0.8)
        assert h[0].dtype == dt and P.same_bits(h[0], f[0].to(dt)) and P.same_bits(h[1], f[1].to(dt))
    with pytest.raises(K.PsndError, match='float64'):
        K.phase_vocoder(a.double(), b.double(), 0.8)
    with pytest.raises(K.PsndError):
        K.phase_vocoder(a.int(), b.int(), 0.8)
    with pytest.raises(K.PsndError):
        K.phase_vocoder(a, b.cpu(), 0.8)
    assert not want[0].requires_grad and not K.phase_vocoder(a.requires_grad_(True), b, 0.8)[0].requires_grad


def test_same_bits_on_poisoned_memory():
    """both outputs come from torch.empty: every slot, the zeros behind a row's frames included, must be written by the call"""
    K = _K()
    frames, re, im, dre, dim = _ragged()
    a, b, fr = _dev(dre).reshape(-1, 3, 70), _dev(dim).reshape(-1, 3, 70), torch.tensor(frames, device=DEV)

    def fn():
        return list(K.phase_vocoder(a, b, 0.8, fr))

    first = P.assert_same_bits(fn)
    assert (first[0][0] == 0).all() and first[0][2].abs().max() > 0.1


def test_two_launches_side_stream_and_graph_capture():
    K = _K()
    ra, ia = R.seeded_spectrum(2, 5, 300, seed=51)
    rb, ib = R.seeded_spectrum(2, 5, 300, seed=52)
    bre, bim = _dev(ra).reshape(2, 5, 300), _dev(ia).reshape(2, 5, 300)
    want_a = [t.clone() for t in K.phase_vocoder(bre, bim, 0.93)]
    again = K.phase_vocoder(bre, bim, 0.93)
    assert all(P.same_bits(g, w) for g, w in zip(again, want_a))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = K.phase_vocoder(bre, bim, 0.93)       # also warms the allocator outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(P.same_bits(g, w) for g, w in zip(on_side, want_a))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = K.phase_vocoder(bre, bim, 0.93)
    graph.replay()
    torch.cuda.synchronize()
    assert all(P.same_bits(g, w) for g, w in zip(out, want_a))
    bre.copy_(_dev(rb).reshape(2, 5, 300)), bim.copy_(_dev(ib).reshape(2, 5, 300))
    graph.replay()
    torch.cuda.synchronize()
    want_b = K.phase_vocoder(bre, bim, 0.93)
    assert all(P.same_bits(g, w) for g, w in zip(out, want_b)) and not P.same_bits(want_b[0], want_a[0])


# ---- the public functions -------------------------------------------------------------------------------------------------------------------
def _tone(f, sr, T, phase=0.4):
    return (0.5 * np.sin(2.0 * np.pi * f * np.arange(T) / sr + phase)).astype(np.float32)


def _peak(y, n_fft):
    inner = y.detach().double().cpu().numpy()[n_fft:-n_fft]
    return int(np.abs(np.fft.rfft(inner * np.hanning(inner.size))).argmax()), inner.size


def _fix(z, n):
    return z[..., :n] if z.shape[-1] >= n else torch.nn.functional.pad(z, (0, n - z.shape[-1]))


@pytest.mark.parametrize('rate', (0.8, 1.25))
def test_time_stretch_on_hip_tensors(rate):
    from pytorch_sound_amd.utils import sound as U
    from pytorch_sound_amd.models.sound import TimeStretch
    from pytorch_sound_amd.models.transforms import STFT
    K = _K()
    sr, T = 22050, 12000
    n = int(round(T / rate))
    freqs = (453.0 * sr / (n - 2048), 1132.25 * sr / (n - 2048))
    x = _dev(np.stack([_tone(freqs[0], sr, T), _tone(freqs[1], sr, T, 1.0)]))
    y = U.time_stretch(x, rate)
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == (2, n) and not y.requires_grad
    for row, f in zip(y, freqs):
        peak, L = _peak(row, 1024)
        assert peak == round(f * L / sr), (peak, f * L / sr)
    stft = STFT(1024, 256)
    re, im = stft.transform_complex(x)
    assert P.same_bits(_fix(stft.inverse_complex(*K.phase_vocoder(re, im, rate)), n).contiguous(), y)
    m = TimeStretch(rate).to(DEV)
    assert P.same_bits(m(x), y) and P.same_bits(m(x[:, None])[:, 0], y)
    h = U.time_stretch(x.half(), rate)
    assert h.dtype == torch.float16 and h.shape == (2, n)
    assert U.time_stretch(x[0], rate).shape == (n,)
    with pytest.raises(K.PsndError, match='float64'):
        U.time_stretch(x.double(), rate)
    # capture: after the calls above nothing is copied from the host
    buf = x.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(buf)
    graph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(out, y)
    buf.copy_(x.flip(0))
    graph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(out, y.flip(0))


@pytest.mark.parametrize('n_steps', (2, -2, 7))
def test_pitch_shift_on_hip_tensors(n_steps):
    from pytorch_sound_amd.utils import sound as U
    from pytorch_sound_amd.models.sound import PitchShift
    K = _K()
    sr, T = 22050, 20000
    x = _dev(_tone(440.0, sr, T))[None]
    y = U.pitch_shift(x, sr, n_steps)
    assert y.is_cuda and y.dtype == torch.float32 and y.shape == (1, T)
    p, q = K.pitch_ratio(n_steps)
    peak, L = _peak(y[0], 1024)
    assert peak == round(440.0 * (p / q) * L / sr), (peak, 440.0 * (p / q) * L / sr)
    z = _fix(K.resample_poly(U.time_stretch(x, q / p), q, p), T).contiguous()
    assert P.same_bits(z, y)
    m = PitchShift(sr, n_steps).to(DEV)
    assert m.taps.is_cuda and P.same_bits(m(x), y)
