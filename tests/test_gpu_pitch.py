"""psnd_pitch.hip on the GPU against the float64 yardstick tests/f0_ref.py: the glide family over every lane seam of the lags, the span
limit, frame-group seams, window variants, edges, ragged rows, non-finite samples, layouts and dtypes, memory hygiene, streams and graph
capture, and the public function.

The comparison rule.  f0_ref gives every frame a margin (how far its nearest decision was from going the other way, relative to the
threshold).  On the frames with a margin of at least 1e-3 the lag must be EQUAL - exact integers, which fixes voicing too.  f0 (kept voiced
frames) and the aperiodicity (kept frames that no non-finite sample decided) are relative errors against float64, bounded by 16 times what
f0_ref's float32 variant with the sum over j reversed shows on the same inputs: that variant is "the same arithmetic in another order",
the factor covers the order of accumulation and FMA contraction.  The bound is computed in the test from the variant and printed; the
kernel's own error is printed beside it and never enters it.  Measured with the variant on the glide family (no GPU involved): f0 at most
8.9e-8 relative (output rounding), aperiodicity at most 3.5e-6, no lag mismatch on the kept frames; the bounds are therefore at most 1.4e-6
and 5.5e-5 (per case: printed).  The kernel, on one MI355X: no lag mismatch on the kept frames, f0 within 1.23e-7, aperiodicity within 3.1e-6."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f0_ref as R  # noqa: E402
import poison as P  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GROUP = 4                   # frames per workgroup of psnd_pitch.hip


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _tone(sr, T, f, sigma=0.01, seed=0):
    """a steady three-harmonic tone with a little noise: float32"""
    ph = 2.0 * np.pi * f * np.arange(T) / float(sr)
    x = (np.sin(ph + 0.2) + 0.8 * np.sin(2.0 * ph + 0.7) + 0.6 * np.sin(3.0 * ph + 1.9)) * (0.9 / 2.4)
    return (x + np.random.RandomState(2000 + seed).randn(T) * sigma).astype(np.float32)


def _refs(x, hop, sr, tau_min, tau_max, W, thr=0.1):
    """float64 yardstick and its float32-reversed variant of one row"""
    return R.track(x, hop, sr, tau_min, tau_max, W, thr), R.track(x, hop, sr, tau_min, tau_max, W, thr, dtype=np.float32, reverse=True)


def _rel(a, b):
    return float(np.abs(a / b - 1.0).max()) if a.size else 0.0


def _compare(got, refs, label, floor=0.0):
    """got: (f0, aperiodicity, lag) arrays of the frames of refs = [(float64, variant)] rows concatenated.  Asserts the rule of the module
    docstring and returns (frames, left out); `floor`: the smallest error the variant's figure is taken as (the small cases, where a handful
    of frames may all round exactly)"""
    f0, ap, lag = (np.concatenate([np.asarray(g[k]) for g in got]) for k in range(3))
    rf, ra, rl, rm = (np.concatenate([r[0][k] for r in refs]) for k in range(4))
    vf, va, vl, _ = (np.concatenate([r[1][k] for r in refs]) for k in range(4))
    assert f0.dtype == np.float32 and ap.dtype == np.float32 and lag.dtype == np.int32 and f0.shape == rf.shape
    keep = rm >= R.KEEP
    voiced = keep & (rl > 0)
    arith = keep & np.isfinite(rm)                      # decided by arithmetic, not by rule 6
    assert np.array_equal(vl[keep], rl[keep]), '%s: the float32 variant of the yardstick disagrees with float64 on a kept frame' % label
    bound_f = 16.0 * max(_rel(vf[voiced], rf[voiced]), floor)
    bound_a = 16.0 * max(_rel(va[arith], ra[arith]), floor)
    err_f, err_a = _rel(f0[voiced].astype(np.float64), rf[voiced]), _rel(ap[arith].astype(np.float64), ra[arith])
    wrong = int((lag[keep] != rl[keep]).sum())
    print('%s: %d frames, %d voiced, %d left out; lag mismatches on kept frames %d; f0 error %.3g (bound %.3g), aperiodicity error %.3g '
          '(bound %.3g)' % (label, rl.size, int((rl > 0).sum()), int((~keep).sum()), wrong, err_f, bound_f, err_a, bound_a))
    assert wrong == 0, '%s: %d kept frames with another lag, first at frame %d' % (label, wrong, int(np.flatnonzero(keep & (lag != rl))[0]))
    assert (f0[keep & (rl == 0)] == 0).all()
    assert err_f <= bound_f and err_a <= bound_a, label
    return rl.size, int((~keep).sum())


def _rows(out, n=None):
    """(f0, ap, lag) device tensors (N, F) -> per-row tuples of numpy arrays"""
    f0, ap, lag = (t.cpu().numpy() for t in out)
    return [(f0[i], ap[i], lag[i]) for i in range(f0.shape[0] if n is None else n)]


@pytest.mark.parametrize('cfg', range(5))
def test_glide_family(cfg):
    """the four configurations the definition was prototyped on and one more at hop 1 (tests/f0_ref.py), the four noise levels of each as the
    four rows of ONE call; at sigma 0 an eighth of the row is scaled by 1e-3.  A case is a configuration: at most 3 % of its frames may be
    left out.  By the yardstick alone, per configuration: 19 of 1004, 0 of 2804, 0 of 244, 0 of 20, 40 of 12004 (0.4 % in all).
    tau_max = 311 / 256 / 40 / 311 / 80: no multiple of 64, a multiple, less than one wave of lags (tau_min 10)."""
    K = _K()
    sr, hop, T, floor = (R.CONFIGS + R.EXTRA)[cfg]
    tau_min, tau_max, W = R.lags(sr, floor)
    assert (tau_min, tau_max, W) == K.yin_lags(sr, floor)
    rows = [R.glide(sr, T, sg, seed=10 * cfg + k, quiet=(T // 2, 5 * T // 8) if sg == 0 else None) for k, sg in enumerate(R.SIGMAS)]
    refs = [_refs(x, hop, sr, tau_min, tau_max, W) for x in rows]
    out = K.yin_f0(_dev(np.stack(rows)), hop, sr, floor)
    assert out[0].shape == (4, T // hop + 1) and out[0].is_cuda
    n, left = _compare(_rows(out), refs, 'glide %r' % ((sr, hop, T, floor),))
    assert left <= R.LEFT_OUT * n
    if cfg != 1:                                        # 700 samples at a span of 768: every frame reaches over an end, none is voiced
        assert sum(int((r[0][2] > 0).sum()) for r in refs) >= n // 8


@pytest.mark.parametrize('hop', [700, 1500])
def test_upper_limit_of_the_issue(hop):
    """tau_max = 960, W = 1920 (48 kHz with a 50 Hz floor) on one short row of 9 or 5 frames: 15 groups of 64 lags, three passes of five"""
    K = _K()
    sr, T = 48000, 6000
    assert K.yin_lags(sr, 50.0) == (60, 960, 1920)
    x = _tone(sr, T, 400.0)                             # a short period: d' is not flat around its minimum, most frames are kept
    refs = [_refs(x, hop, sr, 60, 960, 1920)]
    out = K.yin_f0(_dev(x), hop, sr, 50.0)
    n, left = _compare([tuple(t.cpu().numpy() for t in out)], refs, 'tau_max 960, hop %d' % hop, floor=2.0 ** -24)
    assert ((refs[0][0][3] >= R.KEEP) & (refs[0][0][2] > 0)).sum() >= 2


@pytest.mark.parametrize('hop', [900, 5000])
def test_beyond_64_kib_of_lds(hop):
    """tau_max = 1500, W = 3000 (48 kHz down to 32 Hz): span 4500.  At hop 5000 the four spans lie back to back, 95 KiB with the d' rows - the
    launch asks for more than the default 64 KiB; at hop 900 they overlap (55 KiB)"""
    K = _K()
    sr, T = 48000, 10000
    assert K.yin_lags(sr, 32.0) == (60, 1500, 3000) and 4500 <= K.lib().psnd_yin_max_span()
    x = _tone(sr, T, 300.0, seed=1)
    refs = [_refs(x, hop, sr, 60, 1500, 3000)]
    out = K.yin_f0(_dev(x), hop, sr, 32.0)
    n, left = _compare([tuple(t.cpu().numpy() for t in out)], refs, 'tau_max 1500, hop %d' % hop, floor=2.0 ** -24)
    assert n == T // hop + 1 and ((refs[0][0][3] >= R.KEEP) & (refs[0][0][2] > 0)).any()
    with pytest.raises(K.PsndError, match='span'):
        K.yin_f0(_dev(x), hop, sr, 15.0)                # tau_max = 3200, W = 6400: beyond psnd_yin_max_span


@pytest.mark.parametrize('F', [GROUP - 1, GROUP, GROUP + 1, 2 * GROUP - 1, 2 * GROUP, 2 * GROUP + 1])
def test_frame_group_seams(F):
    """one frame less than, as many as, one more than a multiple of the frames of a workgroup; two rows, so that a group of the second row
    follows a partly filled group of the first"""
    K = _K()
    sr, hop = 8000, 100
    T = (F - 1) * hop + 37
    tau_min, tau_max, W = R.lags(sr, 100.0)
    rows = [_tone(sr, T, 150.0, seed=F), _tone(sr, T, 190.0, seed=F + 1)]
    refs = [_refs(x, hop, sr, tau_min, tau_max, W) for x in rows]
    out = K.yin_f0(_dev(np.stack(rows)), hop, sr, 100.0)
    assert out[0].shape == (2, F)
    _compare(_rows(out), refs, 'F = %d' % F, floor=2.0 ** -24)


@pytest.mark.parametrize('W', [113, 114, 151])
def test_window_variants(W):
    """W = tau_max, the shortest window (span 226, H = 113 odd); span 227; an odd W with an even H"""
    K = _K()
    sr, hop, T = 8000, 64, 1500
    tau_min, tau_max, _ = R.lags(sr, 71.0)
    assert tau_max == 113
    x = R.glide(sr, 4 * T, 0.02)[:T]
    refs = [_refs(x, hop, sr, tau_min, tau_max, W)]
    out = K.yin_f0(_dev(x), hop, sr, frame_length=W)
    n, left = _compare([tuple(t.cpu().numpy() for t in out)], refs, 'W = %d' % W, floor=2.0 ** -24)
    assert left <= 1 and (refs[0][0][2] > 0).sum() >= n // 2
    with pytest.raises(ValueError):
        K.yin_f0(_dev(x), hop, sr, frame_length=112)


def test_edges():
    K = _K()
    f0, ap, lag = K.yin_f0(torch.zeros(0, device=DEV), 256)                  # T = 0: one frame
    assert f0.tolist() == [0.0] and ap.tolist() == [1.0] and lag.tolist() == [0]
    f0, ap, lag = K.yin_f0(torch.zeros(3, 0, device=DEV), 256)
    assert f0.shape == (3, 1) and (f0 == 0).all() and (ap == 1).all() and (lag == 0).all()
    for T, hop in ((100, 256), (700, 100)):                                  # T < hop; T < span = 933
        x = _tone(22050, T, 200.0)
        got = tuple(t.cpu().numpy() for t in K.yin_f0(_dev(x), hop))
        assert got[0].shape == (T // hop + 1,)
        _compare([got], [_refs(x, hop, 22050, 27, 311, 622)], 'T = %d, hop %d' % (T, hop), floor=2.0 ** -24)
    out = K.yin_f0(torch.zeros(0, 500, device=DEV), 100)                     # N = 0: nothing launched
    assert all(t.shape == (0, 6) and t.is_cuda for t in out)
    assert out[0].dtype == torch.float32 and out[2].dtype == torch.int32


def _ragged(sr=8000, hop=50, T=1200):
    lengths = [T, T - 1, hop, 0]
    rows = np.stack([R.glide(sr, 3 * T, 0.02, seed=n)[T:2 * T] for n in range(4)])
    dirty = rows.copy().view(np.uint32)
    for n in range(4):
        dirty[n, lengths[n]:] = 0x7F7F7F7F
    return rows, dirty.view(np.float32), lengths


def test_ragged_batch():
    K = _K()
    sr, hop, T = 8000, 50, 1200
    rows, dirty, lengths = _ragged(sr, hop, T)
    F = T // hop + 1
    x = _dev(dirty)
    one_by_one = [K.yin_f0(_dev(rows[n, :lengths[n]]), hop, sr) for n in range(4)]
    for lens in (lengths, torch.tensor(lengths, device=DEV), torch.tensor(lengths, dtype=torch.int32)):
        f0, ap, lag = K.yin_f0(x, hop, sr, lengths=lens)
        assert f0.shape == (4, F)
        for n in range(4):
            k = lengths[n] // hop + 1
            for got, want, fill in ((f0, one_by_one[n][0], 0.0), (ap, one_by_one[n][1], 1.0), (lag, one_by_one[n][2], 0)):
                assert P.same_bits(got[n, :k], want), (n, k)
                assert (got[n, k:] == fill).all(), n
    tau_min, tau_max, W = R.lags(sr)
    refs = [_refs(rows[n, :lengths[n]], hop, sr, tau_min, tau_max, W) for n in range(4)]
    _compare([tuple(t.cpu().numpy() for t in o) for o in one_by_one], refs, 'ragged rows', floor=2.0 ** -24)
    assert (one_by_one[0][2] > 0).any()


def test_non_finite_samples_zero_exactly_their_frames():
    K = _K()
    sr, hop, T = 22050, 128, 6000
    x = _tone(sr, T, 180.0)
    x[1777], x[4200] = np.nan, -np.inf
    hit = sorted(set(R.spans_with(1777, T, hop, 933) + R.spans_with(4200, T, hop, 933)))
    refs = [_refs(x, hop, sr, 27, 311, 622)]
    assert np.array_equal(np.flatnonzero(np.isinf(refs[0][0][3])), hit) and 12 <= len(hit) <= 16
    got = tuple(t.cpu().numpy() for t in K.yin_f0(_dev(x), hop, sr))
    assert (got[0][hit] == 0).all() and (got[1][hit] == 1).all() and (got[2][hit] == 0).all()
    rest = np.setdiff1d(np.arange(T // hop + 1), hit)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and (got[2][rest] > 0).sum() > rest.size // 2
    _compare([got], refs, 'non-finite samples', floor=2.0 ** -24)


def test_layouts_and_dtypes():
    K = _K()
    sr, hop, T = 8000, 50, 1201
    x = R.glide(sr, 3 * T, 0.02)[T:2 * T]
    big = _dev(x)
    view, aligned = big[1:], big[1:].clone()
    assert view.data_ptr() % 16 == 4 and aligned.data_ptr() % 16 == 0
    want = K.yin_f0(aligned, hop, sr)
    got = K.yin_f0(view, hop, sr)
    assert all(P.same_bits(g, w) for g, w in zip(got, want))
    two = _dev(np.stack([x[:1200], x[:1200][::-1]]))
    inter = torch.empty(1200, 2, device=DEV)
    inter.copy_(two.t())
    assert not inter.t().is_contiguous()
    assert all(P.same_bits(g, w) for g, w in zip(K.yin_f0(inter.t(), hop, sr), K.yin_f0(two, hop, sr)))
    lead = K.yin_f0(two.reshape(2, 1, 1200), hop, sr)
    assert lead[0].shape == (2, 1, 25) and P.same_bits(lead[2][:, 0], K.yin_f0(two, hop, sr)[2])
    for dt in (torch.float16, torch.bfloat16):
        h = two.to(dt)
        assert all(P.same_bits(g, w) for g, w in zip(K.yin_f0(h, hop, sr), K.yin_f0(h.float(), hop, sr)))
    with pytest.raises(K.PsndError, match='float64'):
        K.yin_f0(two.double(), hop, sr)
    with pytest.raises(K.PsndError):
        K.yin_f0(torch.zeros(64, dtype=torch.int32, device=DEV), hop, sr)


def test_same_bits_on_poisoned_memory():
    """the three outputs come from torch.empty: every slot, the fill behind a row's frames included, must be written by the call"""
    K = _K()
    sr, hop, T = 8000, 50, 1200
    rows, dirty, lengths = _ragged(sr, hop, T)
    x, lens = _dev(dirty), torch.tensor(lengths, device=DEV)

    def fn():
        return list(K.yin_f0(x, hop, sr, lengths=lens))

    first = P.assert_same_bits(fn)
    assert (first[2][0] > 0).any() and (first[1][3] == 1).all()


def test_side_stream_and_graph_capture():
    K = _K()
    sr, hop, T = 8000, 50, 1200
    a = np.stack([R.glide(sr, 3 * T, 0.02, seed=n)[T:2 * T] for n in range(2)])
    b = np.stack([_tone(sr, T, 150.0), _tone(sr, T, 210.0, seed=1)])
    buf = _dev(a)
    want_a = [t.clone() for t in K.yin_f0(buf, hop, sr)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = K.yin_f0(buf, hop, sr)                # also warms the allocator outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert all(P.same_bits(g, w) for g, w in zip(on_side, want_a))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = K.yin_f0(buf, hop, sr)
    graph.replay()
    torch.cuda.synchronize()
    assert all(P.same_bits(g, w) for g, w in zip(out, want_a))
    buf.copy_(_dev(b))
    graph.replay()
    torch.cuda.synchronize()
    want_b = K.yin_f0(_dev(b), hop, sr)
    assert all(P.same_bits(g, w) for g, w in zip(out, want_b))
    assert not P.same_bits(want_b[2], want_a[2]) and (want_b[2] > 0).any()


def test_get_f0_on_a_hip_tensor():
    from pytorch_sound_amd.utils import pitch
    K = _K()
    sr, hop, T = 22050, 256, 6000
    x = _dev(np.stack([_tone(sr, T, 130.0), _tone(sr, T, 330.0, seed=1), np.zeros(T, np.float32)]))
    f0 = pitch.get_f0(x, hop, sr)
    assert isinstance(f0, torch.Tensor) and f0.is_cuda and f0.dtype == torch.float32 and f0.shape == (3, T // hop + 1)
    ref = K.yin_f0(x, hop, sr)
    assert P.same_bits(f0, ref[0])
    f0c, ap = pitch.get_f0_with_confidence(x, hop, sr)
    assert P.same_bits(f0c, ref[0]) and P.same_bits(ap, ref[1])
    inner = slice(3, 20)
    got = f0.cpu().numpy()
    assert np.abs(got[0, inner] / 130.0 - 1).max() < 2e-3 and np.abs(got[1, inner] / 330.0 - 1).max() < 2e-3 and (got[2] == 0).all()
    assert pitch.get_f0(x[0], hop, sr).shape == (T // hop + 1,)
