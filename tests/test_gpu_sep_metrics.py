"""psnd_separation.hip on the GPU against the two-pass float64 yardstick tests/sep_ref.py on the same fp32 samples: every seam of the moment
launch, rows that start off a 16-byte boundary, shapes, lengths, kinds, permutation-invariant matching, gradients, non-finite items,
reproducibility and memory hygiene, graph capture, the separator's loss, mixing at an SNR.

Tolerances.  Values: 1e-4 dB wherever the yardstick value is at most 60 dB (asserted for every input used here in tests/test_sep_host.py,
on the CPU).  The derivation: a moment is an fp64 sum whose products are exact, so its relative error is at most (m + d) 2^-53 with m the
longest serial run of additions and d the depth of the tree above it.  The kernel as built: a lane adds at most span / 256 + 1 = 33
samples serially, lanes fold through 6 shuffles, the four waves through 3 additions, and the spans of a row are added serially:
m + d = ceil(T / 8192) + 42 - 45 for the longest seam case here, 204 for a row of 30 s at 44.1 kHz.  The residual energy is a difference of
moments, which amplifies the relative error by 4 * 10^(v / 10); 10 / ln 10 dB per unit of relative error gives 4.34 * 4e6 * 204 * 1.1e-16 =
3.9e-7 dB at 60 dB.  Rounding the value to fp32 at |v| < 128 costs up to 3.8e-6 dB.  1e-4 leaves a factor of 20.  The case near 100 dB
is checked against what the same derivation gives for it (sep_ref.moment_bound_db: 7.9e-4 dB at m + d = 46) and against nothing else;
observed there: see profiles/NOTEBOOK.md.

Gradients: 1e-5 of the row's largest magnitude against the float64 gradient - fp32 rounding of the output (6e-8) plus the error of the
coefficients, which are ratios of the same moments and residuals (below 1e-9 at 60 dB by the derivation above).

Mixing: the gain is a ratio of two moments rounded to fp32 (6e-8 relative), the sample one fp32 fma: 1e-6 of the row's largest magnitude."""
import functools
import gc
import math
import os
import sys
import tempfile

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison as P  # noqa: E402
import sep_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

VALUE_TOL, GRAD_RTOL, MIX_RTOL = 1e-4, 1e-5, 1e-6


def _K():
    from pytorch_sound_amd import kernels
    return kernels


def _M():
    from pytorch_sound_amd.utils import metrics
    return metrics


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _off(a, k):
    """the array on the device, starting 4 k bytes off a 16-byte boundary (an allocation starts on a 512-byte boundary)"""
    flat = torch.zeros(a.size + 4, dtype=torch.float32, device='cuda')
    view = flat[k:k + a.size].view(a.shape)
    view.copy_(_dev(a))
    assert view.data_ptr() % 16 == 4 * k
    return view


@functools.lru_cache(maxsize=None)
def inputs(name):
    return R.case(name)


@functools.lru_cache(maxsize=None)
def reference(name, kind, zm):
    """the yardstick's Reading of a case, computed once and shared"""
    est, tgt, lens, pit = inputs(name)
    return R.measure(est, tgt, kind, zm, lengths=lens, pit=pit)


def _check(got, ref, what, tol=VALUE_TOL):
    value, perm, pair = (v.cpu().numpy() for v in got)
    assert value.dtype == np.float32 and perm.dtype == np.int32 and pair.dtype == np.float32
    assert perm.tolist() == ref.perm.tolist(), what
    err = float(np.max(np.abs(value.astype(np.float64) - ref.value))) if value.size else 0.0
    perr = float(np.max(np.abs(pair.astype(np.float64) - ref.pair))) if pair.size else 0.0
    print('%s: largest error %.3g dB (values), %.3g dB (pairs), largest value %.2f dB' % (what, err, perr, float(np.max(ref.value))))
    assert err <= tol and perr <= tol, what


def _run(name, kind, zm, est=None, tgt=None):
    e, t, lens, pit = inputs(name)
    return _K().sep_metric(_dev(e) if est is None else est, _dev(t) if tgt is None else tgt, kind, zm, None, lens, pit, True, True)


def test_the_library_reports_the_span_the_cases_are_built_on():
    K = _K()
    assert K.sep_span() == R.SPAN and K.sep_max_sources() >= 4


@pytest.mark.parametrize('T', R.SEAM_T)
def test_seams_at_every_start_modulo_16_bytes(T):
    K = _K()
    name = 'seam:%d' % T
    e, t, lens, pit = inputs(name)
    B, S, _ = e.shape
    for ke, kt in ((0, 0), (1, 1), (2, 3), (3, 0)):      # estimates and targets 0, 4, 8, 12 bytes off, together and apart
        de, dt = _off(e, ke), _off(t, kt)
        assert K._sep_rows(de, B, S, T).data_ptr() == de.data_ptr()          # walked where they lie
        for kind, zm in R.CONFIGS:
            _check(_run(name, kind, zm, de, dt), reference(name, kind, zm), '%s off %d/%d %s zero_mean=%d' % (name, ke, kt, kind, zm))


@pytest.mark.parametrize('B,S', R.SHAPES)
def test_shapes_and_mixed_lengths(B, S):
    K = _K()
    name = 'shape:%d:%d' % (B, S)
    e, t, lens, pit = inputs(name)
    assert e.shape[2] % 4 != 0 and (lens is None or {0, 1, e.shape[2] - 1, e.shape[2]} <= set(lens))
    for kind, zm in R.CONFIGS:
        got = _run(name, kind, zm)
        _check(got, reference(name, kind, zm), '%s %s zero_mean=%d' % (name, kind, zm))
        if lens is not None and kind == 'si_sdr':        # what lies behind a length changes nothing, whatever it is
            ge, gt = e.copy(), t.copy()
            for b, ln in enumerate(lens):
                ge[b, :, ln:], gt[b, :, ln:] = (np.nan, 1e30) if b % 2 else (-1e30, np.inf)
            again = _run(name, kind, zm, _dev(ge), _dev(gt))
            assert all(P.same_bits(a, b) for a, b in zip(got, again))
            for b, ln in enumerate(lens):                # and an item equals the item cut out
                if ln > 0:
                    alone = K.sep_metric(_dev(e[b:b + 1, :, :ln]), _dev(t[b:b + 1, :, :ln]), kind, zm)
                    assert float((alone[0] - got[0][b]).abs().max()) <= 2e-5, b


def test_a_dc_offset_of_twice_the_rms():
    e, t, _, _ = inputs('dc')
    rms = float(np.std(t[0, 0]))
    assert abs(float(np.mean(t[0, 0])) / rms - 2.0) < 0.2
    for kind, zm in R.CONFIGS:
        _check(_run('dc', kind, zm), reference('dc', kind, zm), 'dc %s zero_mean=%d' % (kind, zm))
    with_mean, without = reference('dc', 'si_sdr', False).value, reference('dc', 'si_sdr', True).value
    assert float(np.min(np.abs(with_mean - without))) > 1.0                   # the two definitions differ by dBs here, not by rounding


@pytest.mark.parametrize('name', ['pit3', 'pit4'])
def test_planted_permutations_are_found(name):
    K = _K()
    e, t, lens, _ = inputs(name)
    planted = R.S3_PERMS if name == 'pit3' else R.S4_PERM
    for kind, zm in R.CONFIGS:
        got = _run(name, kind, zm)
        assert got[1].tolist() == planted
        _check(got, reference(name, kind, zm), '%s %s zero_mean=%d' % (name, kind, zm))
    # matched as given, the same inputs read the diagonal of the pair matrix, and permute_sources lines the targets up
    value, perm, pair = _run(name, 'si_sdr', True)
    diag = K.sep_metric(_dev(e), _dev(t), 'si_sdr', True, None, lens, False)
    assert P.same_bits(diag, torch.diagonal(pair, dim1=-2, dim2=-1).contiguous())
    lined = _M().permute_sources(_dev(t), perm)
    assert P.same_bits(K.sep_metric(_dev(e), lined, 'si_sdr', True, None, lens), value)
    # `pair` equals the per-pair metric calls
    S = e.shape[1]
    for i in range(S):
        for j in range(S):
            one = K.sep_metric(_dev(e[:, i:i + 1]), _dev(t[:, j:j + 1]), 'si_sdr', True, None, lens)
            assert float((one[:, 0] - pair[:, i, j]).abs().max()) <= VALUE_TOL, (i, j)


def test_an_exact_tie_goes_to_the_lexicographically_first_permutation():
    e, t, lens, _ = inputs('tie')
    assert np.array_equal(e[0, 0], e[0, 1]) and lens[1] == 0
    for kind, zm in R.CONFIGS:
        value, perm, pair = _run('tie', kind, zm)
        assert perm.tolist() == [[1, 2, 0], [0, 1, 2]]                        # [2, 1, 0] scores the same bits; no samples: identity
        assert P.same_bits(pair[0, 0], pair[0, 1])
        _check((value, perm, pair), reference('tie', kind, zm), 'tie %s zero_mean=%d' % (kind, zm))
    assert _run('tie', 'snr', False)[0][1].tolist() == [0.0, 0.0, 0.0]         # eps / eps


# ---- gradients ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grad_inputs(pit, ragged):
    S, T = (3, R.SPAN + 5) if pit else (2, 4101)
    e, t = R.sources(900 + 2 * pit + ragged, 3, S, T, perms=[list(np.roll(np.arange(S), b)) for b in range(3)] if pit else None, dc=0.5)
    rs = np.random.RandomState(7)
    return e, t, ([T, T - 1, T // 3] if ragged else None), rs.randn(3, S), float(rs.randn())


@pytest.mark.parametrize('through', ['loss', 'value', 'both'])
@pytest.mark.parametrize('ragged', [False, True])
@pytest.mark.parametrize('pit', [False, True])
def test_gradients_against_float64_autograd(pit, ragged, through):
    K = _K()
    e, t, lens, gv, gl = grad_inputs(pit, ragged)
    B, S, T = e.shape
    gv, gl = (None if through == 'loss' else gv), (None if through == 'value' else gl)
    for kind, zm in R.CONFIGS:
        ref = R.measure(e, t, kind, zm, lengths=lens, pit=pit)
        assert float(ref.value.max()) <= R.CAP_DB and (not pit or ref.gap > R.GAP_DB)
        want_e, want_t = R.gradients(e, t, kind, zm, ref.perm, lengths=lens, g_value=gv, g_loss=gl)
        de, dt = _dev(e).requires_grad_(True), _dev(t).requires_grad_(True)
        loss, value, perm, _, flag = K.sep_metric_loss(de, dt, kind, zm, None, lens, pit)
        assert perm.tolist() == ref.perm.tolist() and float(flag) == 0.0
        assert abs(float(loss.detach()) + float(ref.value.mean())) <= VALUE_TOL
        total = 0.0
        if gv is not None:
            total = total + (value * _dev(gv.astype(np.float32))).sum()
        if gl is not None:
            total = total + gl * loss
        total.backward()
        for got, want, who in ((de.grad, want_e, 'estimates'), (dt.grad, want_t, 'targets')):
            got = got.double().cpu().numpy()
            top = np.abs(want).max(axis=-1, keepdims=True)
            err = float(np.max(np.abs(got - want) / np.where(top > 0, top, 1.0)))
            print('%s zero_mean=%d pit=%d ragged=%d through %s, %s: %.3g of the row maximum' % (kind, zm, pit, ragged, through, who, err))
            assert err <= GRAD_RTOL
            for b, ln in enumerate(R.lengths_of(lens, B, T)):
                assert not got[b, :, ln:].any() and not np.signbit(got[b, :, ln:]).any()          # exactly zero behind the length
                assert np.abs(got[b, :, :ln]).max() > 0.0
        if kind == 'si_sdr' and zm:                      # the estimates alone: the same bits, no target gradient formed
            only = _dev(e).requires_grad_(True)
            loss2, value2, _, _, _ = K.sep_metric_loss(only, _dev(t), kind, zm, None, lens, pit)
            (g,) = torch.autograd.grad((gl if gl is not None else 0.0) * loss2 + ((value2 * _dev(gv.astype(np.float32))).sum() if gv is not None else 0.0), only)
            assert P.same_bits(g, de.grad)


def test_a_non_finite_item_reads_nan_and_leaves_the_others_bits():
    K = _K()
    e, t = R.sources(950, 3, 2, R.SPAN + 9, perms=[[1, 0], [0, 1], [1, 0]])
    lens = [R.SPAN + 9, R.SPAN + 2, 5000]

    def run(est, tgt):
        de, dt = _dev(est).requires_grad_(True), _dev(tgt).requires_grad_(True)
        loss, value, perm, pair, flag = K.sep_metric_loss(de, dt, 'si_sdr', True, None, lens, True, True)
        loss.backward()
        return loss.detach(), value.detach(), perm, pair, flag, de.grad, dt.grad

    base = run(e, t)
    assert float(base[4]) == 0.0 and base[2].tolist() == [[1, 0], [0, 1], [1, 0]] and bool(torch.isfinite(base[0]))
    for where, bad, at in (('est', np.nan, R.SPAN + 1), ('tgt', np.inf, 0), ('est', -np.inf, 4097)):
        be, bt = e.copy(), t.copy()
        (be if where == 'est' else bt)[1, 1, at] = bad
        loss, value, perm, pair, flag, ge, gt = run(be, bt)
        assert math.isnan(float(loss)) and float(flag) == 1.0
        assert bool(torch.isnan(value[1]).all()) and bool(torch.isnan(pair[1]).all()) and perm[1].tolist() == [0, 1]
        for b in (0, 2):
            assert P.same_bits(value[b], base[1][b]) and P.same_bits(perm[b], base[2][b]) and P.same_bits(pair[b], base[3][b])
        # the gradient through the NaN loss: NaN before the bad item's length, exactly 0 behind every length
        for g in (ge, gt):
            assert bool(torch.isnan(g[1, :, :lens[1]]).all())
            for b in range(3):
                assert not bool(g[b, :, lens[b]:].any())
    be = e.copy()
    be[1, 0, lens[1]] = np.nan                           # behind the item's length: not a sample of it
    assert all(P.same_bits(a, b) for a, b in zip(run(be, t)[:5], base[:5]))
    # through the values, the good items' gradients keep their bits next to a bad one
    be[1, 0, 3] = np.nan
    de = _dev(be).requires_grad_(True)
    value = K.sep_metric(de, _dev(t), 'si_sdr', True, None, lens, True)
    w = torch.tensor([[1.0, 1.0], [0.0, 0.0], [1.0, 1.0]], device='cuda')
    (g_bad,) = torch.autograd.grad((torch.nan_to_num(value) * w).sum(), de)
    dg = _dev(e).requires_grad_(True)
    (g_good,) = torch.autograd.grad((K.sep_metric(dg, _dev(t), 'si_sdr', True, None, lens, True) * w).sum(), dg)
    assert P.same_bits(g_bad[0], g_good[0]) and P.same_bits(g_bad[2], g_good[2])


def test_two_runs_and_poisoned_memory_give_the_same_bits():
    K = _K()
    e, t, lens, _ = inputs('pit4')
    x, z = _dev(e[:, 0]), _dev(t[:, 1])
    de, dt = _dev(e), _dev(t)
    gv = _dev(np.random.RandomState(3).randn(2, 4).astype(np.float32))

    def run():
        a, b = de.clone().requires_grad_(True), dt.clone().requires_grad_(True)
        loss, value, perm, pair, flag = K.sep_metric_loss(a, b, 'si_sdr', True, None, lens, True, True)
        ga, gb = torch.autograd.grad(loss + (value * gv).sum(), [a, b])
        snr = K.sep_metric(de, dt, 'snr', False, None, lens, False)
        return [loss.detach(), value.detach(), perm, pair, flag, ga, gb, snr, K.mix_at_snr(x, z, 7.0, lengths=lens, return_gain=True)]

    first, second = P.to_cpu(run()), P.to_cpu(run())
    assert not P.differences([first, second], (0, 1))
    P.assert_same_bits(run)


def test_nothing_outside_the_outputs_is_written():
    K = _K()
    from pytorch_sound_amd._lib import lib, on
    e, t, lens, _ = inputs('pit4')
    B, S, T = e.shape
    de, dt, dl = _dev(e), _dev(t), torch.tensor(lens, device='cuda')
    nscr, nst = int(lib().psnd_sep_scratch_bytes(B, S, T)) // 8, int(lib().psnd_sep_stats_doubles(B, S))
    guard = 64
    outs = {}
    for fill in (0.0, math.nan):
        d = torch.full((guard + nscr + guard + nst + guard,), fill, dtype=torch.float64, device='cuda')
        f = torch.full((guard + B * S + guard + B * S * S + guard + 2 + guard + 2 * B * S * T + guard,), fill, device='cuda')
        perm = torch.full((guard + B * S + guard,), -7, dtype=torch.int32, device='cuda')
        d0, f0 = d.clone(), f.clone()
        scratch, stats = d[guard:guard + nscr], d[2 * guard + nscr:2 * guard + nscr + nst]
        o = guard
        value = f[o:o + B * S]
        o += B * S + guard
        pair = f[o:o + B * S * S]
        o += B * S * S + guard
        loss, flag = f[o:o + 1], f[o + 1:o + 2]
        o += 2 + guard
        ge, gt = f[o:o + B * S * T], f[o + B * S * T:o + 2 * B * S * T]
        with on(de.device) as hip:
            hip.psnd_sep_metric_fwd(de, dt, B, S, T, dl, 1, 1, R.EPS, 1, scratch, stats, value, perm[guard:guard + B * S], pair, loss, flag)
            hip.psnd_sep_metric_bwd(de, dt, B, S, T, 1, 1, R.EPS, stats, perm[guard:guard + B * S], loss, None, ge, gt)
        torch.cuda.synchronize()
        wd = torch.zeros_like(d, dtype=torch.bool)
        wd[guard:guard + nscr] = True
        wd[2 * guard + nscr:2 * guard + nscr + nst] = True
        assert P.same_bits(d[~wd], d0[~wd])
        wf = torch.zeros_like(f, dtype=torch.bool)
        for lo, n in ((guard, B * S), (2 * guard + B * S, B * S * S), (3 * guard + B * S + B * S * S, 2), (o, 2 * B * S * T)):
            wf[lo:lo + n] = True
        assert P.same_bits(f[~wf], f0[~wf]) and bool(torch.isfinite(f[wf]).all())
        assert bool((perm[:guard] == -7).all()) and bool((perm[guard + B * S:] == -7).all())
        assert perm[guard:guard + B * S].view(B, S).tolist() == R.S4_PERM and bool(torch.isfinite(stats).all())
        outs[fill == 0.0] = (f[wf].clone(), stats.clone())
    assert P.same_bits(outs[True][0], outs[False][0]) and P.same_bits(outs[True][1], outs[False][1])
    assert P.same_bits(outs[True][0][:B * S].view(B, S), K.sep_metric(de, dt, 'si_sdr', True, None, lens, True))


# ---- capture, the loss module, the separator ----------------------------------------------------------------------------------------------
def test_graph_capture_of_forward_and_backward_replays_to_the_eager_bits():
    from pytorch_sound_amd.models.sound import SeparationLoss
    a = R.sources(960, 2, 3, R.SPAN + 5, perms=[[2, 0, 1], [0, 2, 1]])
    b = R.sources(961, 2, 3, R.SPAN + 5, perms=[[1, 0, 2], [2, 1, 0]])
    lens = torch.tensor([R.SPAN + 5, 6000], device='cuda')
    crit = SeparationLoss('si_sdr', pit=True)
    est, tgt = _dev(a[0]).requires_grad_(True), _dev(a[1]).requires_grad_(True)

    def run():
        loss = crit(est, tgt, lens)
        ge, gt = torch.autograd.grad(loss, [est, tgt])
        return loss.detach(), loss.psnd_nan_flag, crit.last_perm, crit.last_value, ge, gt

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                            # warm the allocator outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for data, planted in ((a, [[2, 0, 1], [0, 2, 1]]), (b, [[1, 0, 2], [2, 1, 0]])):
        with torch.no_grad():
            est.copy_(_dev(data[0]))
            tgt.copy_(_dev(data[1]))
        graph.replay()
        torch.cuda.synchronize()
        got = P.to_cpu(captured)
        assert got[2].tolist() == planted                # the permutation is chosen on the device, inside the graph
        assert not P.differences([P.to_cpu(run()), got], (0, 1))


@pytest.fixture
def collected():
    """models and Trainers sit in reference cycles: release their device memory when the case ends, not in the middle of a later test"""
    yield
    gc.collect()
    torch.cuda.synchronize()


def _separator():
    from pytorch_sound_amd.models.separator import ConvSeparator
    from pytorch_sound_amd.models.transforms import STFT
    torch.manual_seed(5)
    return ConvSeparator(129, 32, 1).cuda(), STFT(256, 64).cuda()


def test_the_loss_on_the_separators_waveform_reaches_the_parameters(collected):
    from pytorch_sound_amd.models.sound import SeparationLoss
    from pytorch_sound_amd.trainer import Trainer
    model, stft = _separator()
    g = torch.Generator().manual_seed(2)
    clean = (torch.randn(4, 4096, generator=g) * 0.1).cuda()
    noisy = clean + (torch.randn(4, 4096, generator=g) * 0.05).cuda()
    out = model.separate(noisy, stft)
    for crit, est, tgt in ((SeparationLoss('si_sdr'), out, clean[:, :out.shape[1]]),
                           (SeparationLoss('snr', pit=True), out.view(2, 2, -1), clean[:, :out.shape[1]].reshape(2, 2, -1).flip(1))):
        model.zero_grad()
        loss = crit(est, tgt)
        assert loss.shape == () and loss.dtype == torch.float32 and bool(torch.isfinite(loss))
        assert Trainer._nan_flag(loss) is loss.psnd_nan_flag and float(loss.psnd_nan_flag) == 0.0
        assert crit.last_perm.shape == crit.last_value.shape == est.reshape(est.shape[0], -1, est.shape[-1]).shape[:2]
        assert abs(float(loss) + float(crit.last_value.mean())) <= 1e-5
        loss.backward(retain_graph=True)
        for name, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0.0, name


def _train(graph, steps=6):
    from pytorch_sound_amd.models.sound import SeparationLoss
    from pytorch_sound_amd.trainer import Trainer, LogType
    model, stft = _separator()
    crit = SeparationLoss('si_sdr', pit=True)
    g = torch.Generator().manual_seed(3)
    pool = [(torch.randn(4, 4096, generator=g) * 0.1, torch.randn(4, 4096, generator=g) * 0.1) for _ in range(steps)]

    class T(Trainer):
        def forward(self, noisy, clean, is_logging=False):
            out = self.model.separate(noisy, stft)
            loss = crit(out.view(2, 2, -1), clean[:, :out.shape[1]].reshape(2, 2, -1))    # two "sources" per item, matched on the device
            return loss, {'loss': (loss, LogType.SCALAR)}

    opt = torch.optim.Adam(model.parameters(), lr=1e-3, fused=True)
    tr = T(model, opt, pool, pool, max_step=10 ** 9, valid_max_step=1, save_interval=10 ** 9, log_interval=10 ** 9,
           save_dir=tempfile.mkdtemp(prefix='psnd_sepmetric_'), seed=11)
    tr.graph_steps = graph
    model.train()
    for i in range(1, steps + 1):
        tr.step = i
        tr.train(i)
    torch.cuda.synchronize()
    tr._poll_nan_log(block=True)
    return [p.detach().float().clone() for p in model.parameters()], len(getattr(tr, '_graphs', {}))


def test_a_pit_training_step_is_captured_by_the_trainer(collected):
    eager, n0 = _train(False)
    graph, n1 = _train('auto')
    assert n0 == 0 and n1 == 1                           # 'auto' refuses a step that synchronises with the host: this one does not
    for a, b in zip(eager, graph):
        assert bool(torch.isfinite(b).all()) and float((a - b).abs().max()) <= 2e-2 * (float(a.abs().max()) + 1e-6)


# ---- layouts, dtypes, the public functions ----------------------------------------------------------------------------------------------------
def test_layouts_dtypes_and_the_public_functions():
    K, M = _K(), _M()
    e, t = R.sources(970, 6, 2, 2051, perms=[[1, 0]] * 6)
    de, dt = _dev(e), _dev(t)
    value, perm = M.pit(de, dt)
    assert value.shape == perm.shape == (6, 2) and perm.dtype == torch.int32 and perm.tolist() == [[1, 0]] * 6
    # leading shapes
    v2, p2 = M.pit(de.view(2, 3, 2, -1), dt.view(2, 3, 2, -1), lengths=torch.full((2, 3), 2051))
    assert v2.shape == (2, 3, 2) and P.same_bits(v2.reshape(6, 2), value) and P.same_bits(p2.reshape(6, 2), perm)
    # rows of any leading shape; the torchmetrics defaults
    for fn, kind, zm in ((M.snr, 'snr', False), (M.si_sdr, 'si_sdr', True), (M.sd_sdr, 'sd_sdr', False)):
        got = fn(de, dt)
        assert got.shape == (6, 2) and got.dtype == torch.float32
        ref = np.array([[R.pair_value(kind, e[b, i].astype(np.float64), t[b, i].astype(np.float64), zm) for i in range(2)] for b in range(6)])
        assert float(np.max(np.abs(got.double().cpu().numpy() - ref))) <= VALUE_TOL
        assert fn(de[0, 0], dt[0, 0]).shape == ()
        cut = fn(de[:, 0], dt[:, 0], lengths=[2051, 1000, 1, 0, 7, 2050])
        assert abs(float(cut[1]) - R.pair_value(kind, e[1, 0, :1000].astype(np.float64), t[1, 0, :1000].astype(np.float64), zm)) <= VALUE_TOL
    # a view that cannot be walked where it lies is copied; other float dtypes are cast
    wide = torch.zeros(6, 2, 2052, device='cuda')
    wide[..., 1:] = de
    assert P.same_bits(M.pit(wide[..., 1:], dt)[0], value)
    assert P.same_bits(M.pit(de.double(), dt.double())[0], value)
    hb = M.pit(de.bfloat16(), dt.bfloat16())
    assert P.same_bits(hb[0], M.pit(de.bfloat16().float(), dt.bfloat16().float())[0])
    grad = de.bfloat16().requires_grad_(True)
    M.si_sdr(grad, dt.bfloat16()).sum().backward()
    assert grad.grad.dtype == torch.bfloat16 and bool(torch.isfinite(grad.grad).all())
    # nothing to launch
    assert M.pit(de[:0], dt[:0])[0].shape == (0, 2)
    empty = K.sep_metric(de[..., :0], dt[..., :0], 'snr')
    assert empty.shape == (6, 2) and not bool(empty.any())
    with pytest.raises(K.PsndError):
        K.sep_metric(torch.zeros(1, 5, 100, device='cuda'), torch.zeros(1, 5, 100, device='cuda'), 'snr')
    with pytest.raises(K.PsndError):
        K.sep_metric(de, dt[:, :1], 'snr')
    with pytest.raises(ValueError):
        K.sep_metric(de, dt, 'sdr')


# ---- mixing at an SNR -------------------------------------------------------------------------------------------------------------------------
def test_add_noise_against_the_yardstick():
    K = _K()
    from pytorch_sound_amd.utils import sound as U
    rs = np.random.RandomState(11)
    T = R.SPAN + 7
    wav = (0.1 * rs.randn(6, T)).astype(np.float32)
    noise = (0.5 * rs.randn(6, T)).astype(np.float32)
    wav[2] = 0.0                                         # silent speech
    noise[3] = 0.0                                       # silent noise
    noise[4, R.SPAN + 1] = np.nan                        # a non-finite row
    snr = np.array([20.0, -5.0, 10.0, 10.0, 10.0, 0.0], dtype=np.float32)
    lens = [T, T - 1, T, T, T, 4097]
    for k in range(4):                                   # every start modulo 16 bytes
        for ln in (None, lens):
            want, gain = R.mix(wav, noise, snr, ln)
            y, g = K.mix_at_snr(_off(wav, k), _off(noise, (k + 1) % 4), _dev(snr), lengths=ln, return_gain=True)
            assert y.dtype == torch.float32 and y.shape == wav.shape and g.shape == (6,)
            got = y.double().cpu().numpy()
            top = np.abs(want).max(axis=-1, keepdims=True)
            err = float(np.max(np.abs(got - want) / np.where(top > 0, top, 1.0)))          # NaN never equals: the non-finite row is compared by bits below
            gerr = float(np.max(np.abs(g.double().cpu().numpy() - gain) / np.maximum(gain, 1e-30)))
            print('off %d lengths %s: mix %.3g, gain %.3g' % (k, ln is not None, err, gerr))
            assert err <= MIX_RTOL and gerr <= MIX_RTOL
            assert g[2:5].tolist() == [0.0, 0.0, 0.0]
            for r in (2, 3, 4):                          # unchanged, bit for bit (the NaN included)
                assert P.same_bits(y[r], _dev(wav[r]))
            for r, ll in enumerate(R.lengths_of(ln, 6, T)):
                assert np.array_equal(got[r, ll:], wav[r, ll:].astype(np.float64))
            for r in (0, 1, 5):                          # the achieved SNR over the row's length
                ll = R.lengths_of(ln, 6, T)[r]
                achieved = R.pair_value('snr', got[r, :ll], wav[r, :ll].astype(np.float64), False, 0.0)
                assert abs(achieved - float(snr[r])) <= 1e-3, (r, achieved)
    # one SNR for every row, the public function, in place
    x = _dev(wav)
    y = U.add_noise(x, _dev(noise), 12.0, lengths=lens)
    assert y.data_ptr() != x.data_ptr() and np.array_equal(x.cpu().numpy(), wav)
    want, _ = R.mix(wav, noise, 12.0, lens)
    assert float(np.max(np.abs(y.double().cpu().numpy() - want))) <= MIX_RTOL
    same = K.mix_at_snr(x, _dev(noise), 12.0, lengths=lens, out=x)
    assert same is x and P.same_bits(x, y)
    # dtypes and shapes come back as they went in; no gradient
    hb = U.add_noise(_dev(wav).view(2, 3, T).half(), _dev(noise).view(2, 3, T).half(), _dev(snr).view(2, 3))
    assert hb.dtype == torch.float16 and hb.shape == (2, 3, T)
    with pytest.raises(K.PsndError):
        U.add_noise(_dev(wav).requires_grad_(True), _dev(noise), 10.0)
    with pytest.raises(K.PsndError):
        U.add_noise(_dev(wav), _dev(noise), _dev(snr[:4]))
    assert U.add_noise(x[:, :0], _dev(noise)[:, :0], 3.0).shape == (6, 0)


# ---- sizes --------------------------------------------------------------------------------------------------------------------------------------
def test_the_full_size_case():
    """(4, 2, 30 s at 44.1 kHz) with lengths and matching, against the yardstick"""
    e, t, lens, pit = inputs('full')
    de, dt = _dev(e).requires_grad_(True), _dev(t)
    for kind, zm in R.FULL_CONFIGS:
        _check(_run('full', kind, zm, de.detach(), dt), reference('full', kind, zm), 'full %s zero_mean=%d' % (kind, zm))
    loss, value, perm, _, _ = _K().sep_metric_loss(de, dt, 'si_sdr', True, None, lens, True)
    loss.backward()
    ref = reference('full', 'si_sdr', True)
    want = R.gradients(e, t, 'si_sdr', True, ref.perm, lengths=lens, g_loss=1.0)[0]
    got = de.grad.double().cpu().numpy()
    err = float(np.max(np.abs(got - want) / np.abs(want).max(axis=-1, keepdims=True)))
    print('full size gradient: %.3g of the row maximum' % err)
    assert err <= GRAD_RTOL and not got[2, :, lens[2]:].any()


def test_near_100_db_against_the_bound_of_the_derivation():
    K = _K()
    e, t = R.high_ratio_case()
    m_plus_d = -(-e.shape[2] // R.SPAN) + 42
    for kind, zm in R.CONFIGS:
        want = R.measure(e, t, kind, zm).value.item()
        got = float(K.sep_metric(_dev(e), _dev(t), kind, zm))
        bound = R.moment_bound_db(want, m_plus_d)
        print('%s zero_mean=%d: %.6f dB, yardstick %.6f, error %.3g, bound %.3g (m + d = %d)' % (kind, zm, got, want, abs(got - want), bound, m_plus_d))
        assert 95.0 < want < 105.0 and abs(got - want) <= bound
