"""psnd_griffinlim.hip and kernels.griffinlim on the GPU against the float64 yardstick tests/gl_ref.py: chunk seams, with and without the
previous spectrum, the per-chunk sums, exact zeros, tiny and huge |t|, ragged items over planted NaNs, memory hygiene, aliasing, layouts and
dtypes, the start kernel, and the whole loop (composition by hand, n_iter and momentum against the float64 CPU loop, the fixed point, the
convergence measure, a tone, the public functions, a side stream, graph capture, no library op).

The comparison rule (the one of tests/test_gpu_phase_vocoder.py).  EVERY element is compared.  The error of a case is
max |got - ref| / max |ref| against the float64 yardstick on the same float32 inputs.  The bound is 16 times the error of the yardstick's own
float32 variant on the same case (every operation rounded to float32 with numpy's correctly rounded functions; for the loop the float32 CPU
loop through the host transforms), with a floor of one float32 rounding (2^-24): the factor covers the device library's elementary functions
(hypotf, sincosf) and another order of accumulation (the fused multiply-add of t, the tree of the sums, the transforms' kernels).  The bound
is computed in the test from the variant and printed; the kernel's own error is printed beside it and never enters it.  A loop case is
admissible only if its variant error is below 1e-3 (asserted): beyond that the iteration amplifies rounding and no bound of this kind
means anything.

Variant errors on the cases of this file (no GPU involved): 6e-8 to 7.3e-7 for the step, 6e-8 to 2e-6 for its sums (added in float32 in
element order), 1.8e-7 to 6.6e-6 for the loop after 0 to 8 iterations.

Measured on one MI355X (kernel error / bound).  Step, chunk seams (K F = 1, 2047, 2048, 2049, 4097; N = 1 and 3; with and without P;
alpha 0 and 0.497): at most 1.3e-7 / 1.4e-6; its sums at most 4.4e-7 / 3.8e-6 (three single elements, where |C| - S cancels; 1.1e-7 /
1.3e-5 on whole chunks).  Zeros 1.1e-7 / 1.4e-6; |t| = 1e-18 9.8e-8 / 1.6e-6; |t| = 1e30 1.1e-7 / 1.3e-6; ragged 1.4e-7 / 3.8e-6.
Start with a phase at most 8.3e-8 / 1.3e-6, without one exact.  Loop against the float64 CPU loop: n_iter 0 2.3e-7 / 2.8e-6 and
1.9e-7 / 3.4e-6; STFT(256, 64) n_iter 1, 2, 4, 8 at momentum 0: 5.1e-6 / 2.8e-5, 2.4e-6 / 1.5e-5, 1.8e-6 / 2.4e-5, 6.5e-6 / 3.7e-5, at
momentum 0.99: 5.1e-6 / 2.8e-5, 2.4e-6 / 1.5e-5, 5.5e-6 / 8.3e-5, 1.9e-5 / 1.1e-4; STFT(400, 100) at momentum 0: 1.0e-6 / 2.1e-5,
2.2e-6 / 2.7e-5, 4.9e-6 / 4.3e-5, 9.6e-6 / 4.4e-5 (the worst ratio, 0.22), at momentum 0.99: 1.0e-6 / 2.1e-5, 2.5e-6 / 2.8e-5,
7.7e-6 / 5.7e-5, 1.3e-5 / 9.2e-5.  Fixed point against the input waveform 3.8e-7 / 5.1e-6 and 3.2e-7 / 5.1e-6.  Convergence measure at
most 7.4e-8 / 9.5e-7."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gl_ref as R  # noqa: E402
import poison as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ONE_ROUNDING = 2.0 ** -24
ALPHA = 0.99 / 1.99


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(ts):
    return tuple(t.detach().double().cpu().numpy() for t in ts)


def _shape_of(M):
    """(K, F) with K F = M, K the smallest factor above 1 (1 for a prime)"""
    for k in range(2, int(M ** 0.5) + 1):
        if M % k == 0:
            return k, M // k
    return 1, M


def _bound(var, ref):
    return 16.0 * max(R.rel_err(var, ref), ONE_ROUNDING)


_PART = {}


def _partials(key, S, cr, ci, frames=None):
    """(float64 sums, float32 variant) per chunk, computed once per key and left unchanged"""
    if key not in _PART:
        C = _K().gl_chunk()
        _PART[key] = (R.partial(S, cr, ci, C, frames), R.partial(S, cr, ci, C, frames, dtype=np.float32))
        for a in _PART[key]:
            a.setflags(write=False)
    return _PART[key]


def _check_step(label, planes, alpha, with_p, frames=None, part_key=None, sums=True):
    K = _K()
    S, cr, ci, pr, pi = planes
    if not with_p:
        pr = pi = None
    a32 = float(np.float32(alpha))                       # the kernel takes alpha as a float: the same number for the yardstick
    ref = R.step(S, cr, ci, pr, pi, a32, frames=frames)
    var = R.step(S, cr, ci, pr, pi, a32, frames=frames, dtype=np.float32)
    out = K.griffinlim_step(_dev(S), _dev(cr), _dev(ci), _dev(pr), _dev(pi), alpha, frames=frames, partial=True)
    assert out[0].dtype == torch.float32 and out[0].is_cuda and out[0].shape == S.shape
    got = _np(out[:2])
    bound, err = _bound(var, ref), R.rel_err(got, ref)
    print('%s: %s alpha %.3g P %s: kernel error %.3g, bound %.3g (variant %.3g)' % (label, S.shape, alpha, with_p, err, bound, bound / 16.0))
    assert err <= bound, label
    if not sums:
        return got, ref, out[2].double().cpu().numpy()
    pref, pvar = _partials(part_key or label, S, cr, ci, frames)
    pgot = out[2].double().cpu().numpy()
    assert pgot.shape == pref.shape == (S.shape[0], K.gl_chunks(S.shape[1], S.shape[2]), 2)
    for j, name in enumerate(('sum (|C| - S)^2', 'sum S^2')):
        pb, pe = _bound(pvar[..., j], pref[..., j]), R.rel_err(pgot[..., j], pref[..., j])
        print('%s: %s: kernel error %.3g, bound %.3g (variant %.3g)' % (label, name, pe, pb, pb / 16.0))
        assert pe <= pb, (label, name)
    return got, ref, pgot


# ---- the step kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ('1', 'C-1', 'C', 'C+1', '2C+1'))
def test_chunk_seams(which):
    """K F around the elements of a workgroup; N = 1 and N = 3 (with an odd K F the items start off a 16-byte boundary); with and without P,
    alpha 0 and 0.99 / 1.99"""
    C = _K().gl_chunk()
    M = {'1': 1, 'C-1': C - 1, 'C': C, 'C+1': C + 1, '2C+1': 2 * C + 1}[which]
    Kb, F = _shape_of(M)
    for N in (1, 3):
        planes = R.planes(N, Kb, F, seed=M % 97 + N)
        for with_p in (False, True):
            for alpha in (0.0, ALPHA):
                _check_step('seam %s N=%d' % (which, N), planes, alpha, with_p, part_key='seam %s N=%d' % (which, N))


def test_exact_zeros():
    """t = 0 gives exactly (0, 0), S = 0 too; -0 inputs included"""
    K = _K()
    S, cr, ci, pr, pi = R.planes(2, 7, 150, seed=11)
    cr[0, 1, 10:40] = ci[0, 1, 10:40] = 0.0              # t = 0 without P
    cr[0, 1, 20:25] = -0.0
    S[1, 3, 50:90] = 0.0                                 # S = 0
    S[1, 3, 60:65] = -0.0
    got, ref, _ = _check_step('zeros, no P', (S, cr, ci, pr, pi), 0.0, False)
    for g in got:
        assert (g[0, 1, 10:40] == 0).all() and (g[1, 3, 50:90] == 0).all()
    # t = 0 with P: C = alpha P exactly (alpha = 0.5: the product is exact)
    pr2, pi2 = (2.0 * cr).astype(np.float32), (2.0 * ci).astype(np.float32)
    out = K.griffinlim_step(_dev(S), _dev(cr), _dev(ci), _dev(pr2), _dev(pi2), 0.5)
    assert bool((out[0] == 0).all()) and bool((out[1] == 0).all())
    assert np.abs(got[0]).max() > 0.1


@pytest.mark.parametrize('size', (1e-18, 1e30))
def test_tiny_and_huge_t_stay_finite(size):
    """the quotient is taken first: |t| = 1e30 does not overflow (a product S t would, and so would t_re^2 + t_im^2); |t| = 1e-18 lies
    below eps and gives about S |t| / eps"""
    rs = np.random.RandomState(12)
    S = rs.uniform(0.5, 2.0, (2, 5, 33)).astype(np.float32)
    ang = rs.uniform(-np.pi, np.pi, S.shape)
    cr, ci = (size * np.cos(ang)).astype(np.float32), (size * np.sin(ang)).astype(np.float32)
    pr, pi = (-0.5 * cr).astype(np.float32), (0.25 * ci).astype(np.float32)
    for with_p in (False, True):
        # the sums: checked at 1e-18; at 1e30 (|C| - S)^2 leaves float32 on both sides, as IEEE gives, and only sum S^2 stays finite
        got, ref, pgot = _check_step('|t| = %g' % size, (S, cr, ci, pr, pi), ALPHA, with_p, part_key='|t| = %g' % size, sums=size < 1)
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        mag = np.hypot(got[0], got[1])
        assert (mag <= 1.001 * S).all() and mag.max() > (1e-3 if size < 1 else 0.9)
    assert np.isfinite(pgot[..., 1]).all() and np.isfinite(pgot[..., 0]).all() == (size < 1)


def _ragged(Kb=37, F=70):
    frames = [0, 1, F, F + 9, -2, 33]
    planes = R.planes(len(frames), Kb, F, seed=21)
    dirty = [a.copy() for a in planes]
    for n, fn in enumerate(frames):                     # what lies behind an item's frames must not be read: NaN and Inf there
        fn = min(max(fn, 0), F)
        for j, a in enumerate(dirty):
            a[n, :, fn:] = np.nan if j % 2 == 0 else np.inf
    return frames, planes, dirty


@pytest.mark.parametrize('with_p', (False, True))
def test_ragged_frames(with_p):
    K = _K()
    Kb, F = 37, 70                                       # 2590 elements per item: two chunks
    frames, planes, dirty = _ragged(Kb, F)
    got, ref, pgot = _check_step('ragged', dirty, ALPHA, with_p, frames, part_key='ragged')
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(pgot).all()
    clean_part = R.partial(*planes[:3], K.gl_chunk(), frames)
    assert np.array_equal(clean_part, _PART['ragged'][0])                      # the yardstick's sums leave the invalid part out
    for n, fn in enumerate(frames):
        fn = min(max(fn, 0), F)
        assert (got[0][n, :, fn:] == 0).all() and (got[1][n, :, fn:] == 0).all(), n
        if fn == 0:
            assert (pgot[n] == 0).all()
            continue
        alone = [_dev(a[n:n + 1, :, :fn]) for a in planes]
        if not with_p:
            alone[3] = alone[4] = None
        one = _np(K.griffinlim_step(*alone, ALPHA)[:2])
        assert np.array_equal(one[0][0], got[0][n, :, :fn]) and np.array_equal(one[1][0], got[1][n, :, :fn]), n
    d = [_dev(a) for a in dirty]
    if not with_p:
        d[3] = d[4] = None
    a = K.griffinlim_step(*d, ALPHA, frames=torch.tensor(frames, device=DEV))                   # frames as a device tensor
    b = K.griffinlim_step(*d, ALPHA, frames=torch.tensor(frames, dtype=torch.int32))            # ... and of another integer type
    assert np.array_equal(a[0].double().cpu().numpy(), got[0]) and P.same_bits(a[1], b[1])


def test_same_bits_on_poisoned_memory():
    """the outputs and the sums come from torch.empty: every slot, the zeros behind an item's frames included, must be written by the call"""
    K = _K()
    frames, planes, dirty = _ragged()
    d = [_dev(a) for a in dirty]
    fr = torch.tensor(frames, device=DEV)

    def fn():
        return list(K.griffinlim_step(*d, ALPHA, frames=fr, partial=True)) + list(K.griffinlim_step(d[0], d[1], d[2], frames=fr)) + \
            list(K.griffinlim_start(d[0], d[3], fr)) + list(K.griffinlim_start(d[0], None, fr))

    first = P.assert_same_bits(fn)
    assert (first[0][0] == 0).all() and first[0][2].abs().max() > 0.1 and (first[2][0] == 0).all()


def test_x_may_be_written_over_p():
    K = _K()
    C = K.gl_chunk()
    Kb, F = _shape_of(2 * C + 1)
    planes = [_dev(a) for a in R.planes(3, Kb, F, seed=31)]
    want = K.griffinlim_step(*planes, ALPHA, partial=True)
    p0, p1 = planes[3].clone(), planes[4].clone()
    got = K.griffinlim_step(planes[0], planes[1], planes[2], p0, p1, ALPHA, out=(p0, p1), partial=True)
    assert got[0].data_ptr() == p0.data_ptr() and got[1].data_ptr() == p1.data_ptr()
    assert P.same_bits(got[0], want[0]) and P.same_bits(got[1], want[1]) and P.same_bits(got[2], want[2])
    again = K.griffinlim_step(*planes, ALPHA, partial=True)                    # repeated launches agree bit for bit
    assert all(P.same_bits(g, w) for g, w in zip(again, want))
    o0, o1 = torch.empty_like(p0), torch.empty_like(p1)                        # out without aliasing
    K.griffinlim_step(*planes, ALPHA, out=(o0, o1))
    assert P.same_bits(o0, want[0]) and P.same_bits(o1, want[1])


def test_layouts_and_dtypes():
    K = _K()
    N, Kb, F = 2, 5, 131
    planes = [_dev(a) for a in R.planes(N, Kb, F, seed=41)]
    want = K.griffinlim_step(*planes, ALPHA)
    lead = K.griffinlim_step(*[t.reshape(N, 1, Kb, F) for t in planes], ALPHA)                  # a leading extra axis
    assert lead[0].shape == (N, 1, Kb, F) and P.same_bits(lead[0][:, 0], want[0]) and P.same_bits(lead[1][:, 0], want[1])
    one = K.griffinlim_step(*[t[0] for t in planes], ALPHA)                                     # (K, F): one item
    assert one[0].shape == (Kb, F) and P.same_bits(one[0], want[0][0])
    views = []
    for t in planes:                                                                            # permuted, non-contiguous views
        s = torch.empty(F, Kb, N, device=DEV)
        s.copy_(t.permute(2, 1, 0))
        views.append(s.permute(2, 1, 0))
    assert not views[0].is_contiguous() and torch.equal(views[0], planes[0])
    got = K.griffinlim_step(*views, ALPHA)
    assert P.same_bits(got[0], want[0]) and P.same_bits(got[1], want[1])
    for j in range(5):                                                                          # a base pointer at 4 modulo 16, plane by plane
        big = torch.zeros(N * Kb * F + 1, device=DEV)
        off = big[1:].reshape(N, Kb, F)
        off.copy_(planes[j])
        assert off.data_ptr() % 16 == 4
        moved = list(planes)
        moved[j] = off
        got = K.griffinlim_step(*moved, ALPHA)
        assert P.same_bits(got[0], want[0]) and P.same_bits(got[1], want[1]), j
    big0, big1 = torch.zeros(N * Kb * F + 1, device=DEV), torch.zeros(N * Kb * F + 1, device=DEV)
    o = (big0[1:].reshape(N, Kb, F), big1[1:].reshape(N, Kb, F))                                # ... and the outputs
    K.griffinlim_step(*planes, ALPHA, out=o)
    assert o[0].data_ptr() % 16 == 4 and P.same_bits(o[0], want[0]) and P.same_bits(o[1], want[1]) and float(big0[0]) == 0.0
    for dt in (torch.float16, torch.bfloat16):
        h = [t.to(dt) for t in planes]
        a, b = K.griffinlim_step(*h, ALPHA), K.griffinlim_step(*[t.float() for t in h], ALPHA)
        assert a[0].dtype == dt and P.same_bits(a[0], b[0].to(dt)) and P.same_bits(a[1], b[1].to(dt))
        a, b = K.griffinlim_start(h[0], h[3]), K.griffinlim_start(h[0].float(), h[3].float())
        assert a[0].dtype == dt and P.same_bits(a[0], b[0].to(dt)) and P.same_bits(a[1], b[1].to(dt))
    with pytest.raises(K.PsndError, match='float64'):
        K.griffinlim_step(*[t.double() for t in planes], ALPHA)
    with pytest.raises(K.PsndError):
        K.griffinlim_step(*[t.int() for t in planes], ALPHA)
    with pytest.raises(K.PsndError):
        K.griffinlim_step(planes[0], planes[1], planes[2].cpu())                                # a CPU / HIP mix
    with pytest.raises(K.PsndError):
        K.griffinlim_step(planes[0].cpu(), planes[1], planes[2])
    with pytest.raises(K.PsndError, match='float64'):
        K.griffinlim_start(planes[0].double())
    with pytest.raises(K.PsndError):
        K.griffinlim_start(planes[0], planes[3].cpu())
    with pytest.raises(K.PsndError):
        K.griffinlim_step(*planes, ALPHA, out=(torch.empty(3, device=DEV), torch.empty(3, device=DEV)))
    e = torch.zeros(2, 3, 0, device=DEV)
    assert K.griffinlim_step(e, e, e)[0].shape == (2, 3, 0) and K.griffinlim_start(e)[1].shape == (2, 3, 0)
    assert not K.griffinlim_step(planes[0].clone().requires_grad_(True), planes[1], planes[2])[0].requires_grad


# ---- the start kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_phi', (False, True))
def test_start(with_phi):
    K = _K()
    C = K.gl_chunk()
    for N, (Kb, F) in ((1, (1, 1)), (3, _shape_of(C + 1)), (2, _shape_of(2 * C + 1))):
        S, phi = R.planes(N, Kb, F, seed=51 + N, count=2)
        phi = (3.0 * phi).astype(np.float32) if with_phi else None
        ref, var = R.start(S, phi), R.start(S, phi, dtype=np.float32)
        got = _np(K.griffinlim_start(_dev(S), _dev(phi)))
        bound, err = _bound(var, ref), R.rel_err(got, ref)
        print('start %s phase %s: kernel error %.3g, bound %.3g' % (S.shape, with_phi, err, bound))
        assert err <= bound
        if not with_phi:
            assert np.array_equal(got[0], S.astype(np.float64)) and (got[1] == 0).all()
    frames, planes, dirty = _ragged()
    phi = dirty[3] if with_phi else None
    ref, var = R.start(dirty[0], phi, frames), R.start(dirty[0], phi, frames, dtype=np.float32)
    got = _np(K.griffinlim_start(_dev(dirty[0]), _dev(phi), frames))
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and R.rel_err(got, ref) <= _bound(var, ref)
    for n, fn in enumerate(frames):
        fn = min(max(fn, 0), 70)
        assert (got[0][n, :, fn:] == 0).all() and (got[1][n, :, fn:] == 0).all()


# ---- the loop -------------------------------------------------------------------------------------------------------------------------------
CASES = ((256, 64, 8192), (400, 100, 8000))              # a power of two and the mixed-radix road


@functools.lru_cache(maxsize=None)
def _case(n_fft, hop, T):
    """(stft, clips (2, T), float32 magnitude (2, K, F) of their float64 host spectrum, a float32 random phase, their true phase)"""
    from pytorch_sound_amd.models.transforms import STFT
    stft = STFT(n_fft, hop)
    x = np.stack([R.clip(T, 3), R.clip(T, 4)])
    re, im = stft.transform_complex(torch.from_numpy(x.astype(np.float64)))
    mag = torch.hypot(re, im).float()
    phi = torch.from_numpy(np.random.RandomState(5).uniform(0, 2 * np.pi, tuple(mag.shape)).astype(np.float32))
    return stft, x, mag, phi, torch.atan2(im, re).float()


@functools.lru_cache(maxsize=None)
def _loop_refs(n_fft, hop, T, n_iter, momentum, true_phase=False):
    """(waveform, conv) of the float64 CPU loop of kernels.griffinlim and of the float32 variant loop of the yardstick; computed once"""
    stft, x, mag, phi, true = _case(n_fft, hop, T)
    ph = true if true_phase else phi
    ref = _K().griffinlim(mag.double(), stft, n_iter, momentum, init_phase=ph.double(), return_convergence=True)
    var = R.loop(mag.numpy(), stft, n_iter, momentum, ph.numpy(), dtype=np.float32)
    out = (ref[0].numpy(), ref[1].numpy()), var
    for a in out[0] + out[1]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('n_fft, hop, T', CASES)
def test_loop_is_its_calls_composed_by_hand(n_fft, hop, T):
    K = _K()
    stft, x, mag, phi, _ = _case(n_fft, hop, T)
    S, ph = mag.to(DEV), phi.to(DEV)
    got = K.griffinlim(S, stft, n_iter=3, momentum=0.99, init_phase=ph)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (2, T) and not got.requires_grad
    X, Pv = K.griffinlim_start(S, ph), (None, None)
    for _ in range(3):
        C = stft.transform_complex(stft.inverse_complex(X[0], X[1]))
        X = K.griffinlim_step(S, C[0], C[1], Pv[0], Pv[1], 0.99 / (1.0 + 0.99), 1e-16)
        Pv = C
    assert P.same_bits(stft.inverse_complex(X[0], X[1]), got)
    assert P.same_bits(K.griffinlim(S, stft, n_iter=3, momentum=0.99, init_phase=ph), got)      # and twice the same bits
    assert P.same_bits(K.griffinlim(S, stft, n_iter=3, momentum=0.99, init_phase=ph, length=1000), got[:, :1000].contiguous())
    assert K.griffinlim(S, stft, n_iter=1, init_phase=ph, length=T + 77).shape == (2, T + 77)


@pytest.mark.parametrize('momentum', (0.0, 0.99))
@pytest.mark.parametrize('n_fft, hop, T', CASES)
def test_loop_against_the_float64_cpu_loop(n_fft, hop, T, momentum):
    K = _K()
    stft, x, mag, phi, _ = _case(n_fft, hop, T)
    S, ph = mag.to(DEV), phi.to(DEV)
    for n_iter in (0, 1, 2, 4, 8):
        (ref, _), (var, _) = _loop_refs(n_fft, hop, T, n_iter, momentum)
        got = K.griffinlim(S, stft, n_iter, momentum, init_phase=ph).double().cpu().numpy()
        v = R.rel_err(var, ref)
        bound, err = 16.0 * max(v, ONE_ROUNDING), R.rel_err(got, ref)
        print('STFT(%d, %d) momentum %g n_iter %d: kernel error %.3g, bound %.3g (variant %.3g)' % (n_fft, hop, momentum, n_iter, err, bound, v))
        assert v < 1e-3, 'the case is not admissible'
        assert err <= bound, n_iter


@pytest.mark.parametrize('n_fft, hop, T', CASES)
def test_fixed_point_at_the_true_phase(n_fft, hop, T):
    """momentum 0, 2 iterations from the true phase: the input waveform comes back"""
    K = _K()
    stft, x, mag, _, true = _case(n_fft, hop, T)
    (_, _), (var, _) = _loop_refs(n_fft, hop, T, 2, 0.0, True)
    got = K.griffinlim(mag.to(DEV), stft, 2, 0.0, init_phase=true.to(DEV)).double().cpu().numpy()
    want = x.astype(np.float64)
    bound, err = _bound(var, want), R.rel_err(got, want)
    print('STFT(%d, %d) fixed point against the input waveform: kernel error %.3g, bound %.3g' % (n_fft, hop, err, bound))
    assert err <= bound and bound < 1e-3


@pytest.mark.parametrize('n_fft, hop, T', CASES)
def test_convergence_measure(n_fft, hop, T):
    K = _K()
    stft, x, mag, phi, _ = _case(n_fft, hop, T)
    for momentum in (0.0, 0.99):
        (_, ref), (_, var) = _loop_refs(n_fft, hop, T, 8, momentum)
        y, conv = K.griffinlim(mag.to(DEV), stft, 8, momentum, init_phase=phi.to(DEV), return_convergence=True)
        assert conv.shape == (8, 2) and conv.dtype == torch.float64 and conv.is_cuda
        assert P.same_bits(y, K.griffinlim(mag.to(DEV), stft, 8, momentum, init_phase=phi.to(DEV)))   # asking for it changes no bit of y
        got = conv.cpu().numpy()
        bound, err = _bound(var, ref), R.rel_err(got, ref)
        print('STFT(%d, %d) momentum %g conv: kernel error %.3g, bound %.3g; conv[:, 0] = %s' % (n_fft, hop, momentum, err, bound, got[:, 0].round(4)))
        assert err <= bound
        if momentum == 0.0:
            assert (got[1:] <= got[:-1]).all()
    _, c0 = K.griffinlim(mag.to(DEV), stft, 0, return_convergence=True)
    assert c0.shape == (0, 2)


def _peak(y, n_fft):
    inner = y.detach().double().cpu().numpy()[n_fft:-n_fft]
    return int(np.abs(np.fft.rfft(inner * np.hanning(inner.size))).argmax()), inner.size


def test_a_tone_comes_back_on_its_bin():
    """16 iterations from the magnitude alone (zero first phase) of a pure tone on a bin centre: the spectral peak sits in the right bin"""
    K = _K()
    stft, T, k = _case(256, 64, 8192)[0], 8192, 20
    x = torch.from_numpy((0.5 * np.sin(2 * np.pi * k / 256.0 * np.arange(T) + 0.4)).astype(np.float32))[None].to(DEV)
    re, im = stft.transform_complex(x)
    y = K.griffinlim(torch.hypot(re, im), stft, n_iter=16, rand_init=False)
    peak, L = _peak(y[0], 256)
    assert peak == round(k / 256.0 * L), (peak, k / 256.0 * L)
    assert float(y[0, 256:-256].abs().max()) > 0.25
    # the random start, drawn on the device: reproducible through a generator.  No peak is asserted for it: after 16 iterations stretches
    # of the result still differ in phase, and the peak of the whole clip's spectrum may sit one bin off (seed 3: bin 601 of 600).
    r = K.griffinlim(torch.hypot(re, im), stft, n_iter=16, generator=torch.Generator(DEV).manual_seed(3))
    again = K.griffinlim(torch.hypot(re, im), stft, n_iter=16, generator=torch.Generator(DEV).manual_seed(3))
    assert r.shape == y.shape and bool(torch.isfinite(r).all()) and P.same_bits(r, again) and not P.same_bits(r, y)


def test_public_functions_side_stream_and_graph_capture():
    from pytorch_sound_amd.utils import sound as U
    from pytorch_sound_amd.models.sound import GriffinLim
    K = _K()
    stft, x, mag, phi, _ = _case(256, 64, 8192)
    S, ph = mag.to(DEV), phi.to(DEV)
    want = K.griffinlim(S, stft, n_iter=4, momentum=0.99, init_phase=ph)
    assert P.same_bits(U.griffinlim(S, 4, init_phase=ph), want) and P.same_bits(U.griffinlim(S, 4, 256, 64, 0.99, None, ph), want)
    zero = K.griffinlim(S, stft, n_iter=4, rand_init=False)
    m = GriffinLim(256, 64, n_iter=4, rand_init=False).to(DEV)
    assert P.same_bits(m(S), zero) and P.same_bits(m(S[0]), zero[0]) and P.same_bits(U.griffinlim(S, 4, rand_init=False), zero)
    p2 = GriffinLim(256, 64, n_iter=4, power=2.0, rand_init=False)
    assert P.same_bits(p2(S ** 2), K.griffinlim((S ** 2) ** 0.5, stft, n_iter=4, rand_init=False))
    h = U.griffinlim(S.half(), 2, rand_init=False)
    assert h.dtype == torch.float16 and h.is_cuda and h.shape == (2, 8192)
    with pytest.raises(K.PsndError, match='float64'):
        U.griffinlim(S.double(), 2)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = m(S)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert P.same_bits(on_side, zero)
    # capture: after the calls above nothing is copied from the host; the graph is a straight line of launches
    other = torch.hypot(*stft.transform_complex(torch.from_numpy(np.stack([R.clip(8192, 8), R.clip(8192, 9)])).to(DEV)))
    want_other = m(other)
    buf = S.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(buf)
    graph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(out, zero)
    buf.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    assert P.same_bits(out, want_other) and not P.same_bits(want_other, zero)


FORBIDDEN = ('aten.bmm', 'aten.baddbmm', 'aten.mm.', 'aten.addmm', 'aten._softmax', 'aten.native_group_norm', 'aten.convolution',
             'aten.miopen', 'aten.cudnn', 'aten._fft', 'aten.stft', 'aten.istft', 'aten.hypot', 'aten.div', 'aten.atan2', 'aten.sub',
             'aten.sqrt', 'aten.sum')


class _Forbid(TorchDispatchMode):
    """the dispatch mode of tests/test_gpu_no_library_paths.py, declared again here, with the elementwise ops a loop in library ops would
    take added to the list"""

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if any(name.startswith(f) for f in FORBIDDEN):
            flat = torch.utils._pytree.tree_leaves((args, kwargs or {}))
            if any(isinstance(a, torch.Tensor) and a.is_cuda for a in flat):
                raise AssertionError('library op %s reached with a HIP tensor' % name)
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize('n_fft, hop, T', CASES)
def test_no_library_op_is_reached(n_fft, hop, T):
    K = _K()
    stft, x, mag, phi, _ = _case(n_fft, hop, T)
    S, ph = mag.to(DEV), phi.to(DEV)
    want = K.griffinlim(S, stft, n_iter=3, momentum=0.99, init_phase=ph)
    with _Forbid():
        got = K.griffinlim(S, stft, n_iter=3, momentum=0.99, init_phase=ph)
        zero = K.griffinlim(S, stft, n_iter=2, rand_init=False)
    assert P.same_bits(got, want) and bool(torch.isfinite(zero).all())
    with pytest.raises(AssertionError, match='library op'):
        with _Forbid():
            torch.hypot(S, S)
