"""The mel kernels of the bin-fastest path after their work was resized to the filter bands (psnd_mel.hip: forward = one wave per
(clip, 16 frames, 16 mel bands) with a ring of operand loads, backward = batches of 4 k-steps, then exactly the 1 - 3 left): the
results are the SAME fp32 sums in the same order as before, so every tensor is compared bit for bit with fixtures recorded from the
kernels before the change (tests/golden/mel_bands_*.npz, written by tools/gen_mel_bands_golden.py; they hold the inputs too).

The fixtures of the 80-band filter hold the 173-frame case only: at recording time the outputs of every shorter clip (1 .. 65 frames =
the first frames of the same input) were checked to be the first frames of the 173-frame outputs, bit for bit, so the shorter clips
are compared with that prefix."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import features as ofe

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LOG_NONE, LOG_E = 0, 1
L1_G, L1_COEF = 0.75, 3.0e-5        # gradient of the loss value (device scalar) and the weight / numel factor of the fused L1 backward

# name: filter, clips, frames of the fixture, the clip lengths compared with it, epilogue (log kind, offset, clamp_lo, clamp_hi)
CASES = {
    'slaney80': dict(N=3, F=173, Fs=(1, 15, 16, 17, 63, 64, 65, 173), log=(LOG_E, 1e-6, ofe.db_to_ln(-50), ofe.db_to_ln(30))),
    'mel40': dict(N=3, F=61, Fs=(61,), log=(LOG_E, 1e-6, ofe.db_to_ln(-50), ofe.db_to_ln(30))),
    'dense24': dict(N=2, F=37, Fs=(37,), log=(LOG_NONE, 0.0, -40.0, 55.0)),
    'k17': dict(N=2, F=20, Fs=(20,), log=(LOG_NONE, 0.0, -3.0, 4.0)),
}


def case_filter(name):
    if name == 'slaney80':
        return ofe.mel_filterbank(22050, 1024, 80, 0, 8000).astype(np.float32)
    if name == 'mel40':
        return ofe.mel_filterbank(16000, 512, 40, 50, 7000).astype(np.float32)
    if name == 'dense24':        # every 16-bin group in the band, the last (one bin) included, negative weights
        return np.random.RandomState(24).randn(24, 513).astype(np.float32)
    return np.random.RandomState(17).randn(5, 17).astype(np.float32)


def case_inputs(name):
    """(W, mag (N, F, K), gout (N, M, F)): an all-zero frame, one clip scaled by 3e4, values on both sides of both clamps.  The magnitude
    keeps 8 mantissa bits so that the fixture can hold it in 16 bits per value."""
    c = CASES[name]
    W = case_filter(name)
    M, K = W.shape
    g = np.random.RandomState(c['F'] + M)
    mag = g.randn(c['N'], c['F'], K).astype(np.float32)
    mag = np.abs(mag) * 3 if c['log'][0] == LOG_E else mag
    mag[0, 0, :] = 0
    mag[1] *= 3.0e4
    mag[-1, c['F'] // 2:] *= 1.0e-3
    mag = (mag.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    gout = g.randn(c['N'], M, c['F']).astype(np.float32)
    return W, mag, gout


def bits16(mag):
    return (mag.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def from_bits16(b):
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def l1_bwd_nfk(ref, lin, plan, K_, log):
    from pytorch_sound_amd._lib import lib, check
    from pytorch_sound_amd.kernels import ptr, stream_ptr
    N, M, F_ = lin.shape
    g = torch.tensor([L1_G], dtype=torch.float32, device=DEV)
    gest = torch.empty((N, F_, K_), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        check(lib().psnd_mel_l1_bwd_nfk(ptr(ref), ptr(lin), ptr(g), L1_COEF, N, F_, M, K_, ptr(plan), log[0], log[1], -1.0, log[2], log[3],
                                        ptr(gest), stream_ptr(DEV)), 'psnd_mel_l1_bwd_nfk')
    return gest


def l1_fwd_nfk(mag, ref, plan, M, log, part):
    from pytorch_sound_amd._lib import lib, check
    from pytorch_sound_amd.kernels import ptr, stream_ptr
    N, F_, K_ = mag.shape
    lin = torch.empty((N, M, F_), dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        check(lib().psnd_mel_l1_fwd_nfk(ptr(mag), N, F_, M, K_, ptr(plan), log[0], log[1], -1.0, log[2], log[3], ptr(ref), ptr(lin),
                                        ptr(part), stream_ptr(DEV)), 'psnd_mel_l1_fwd_nfk')
    return lin


def run_forward(plan, M, mag, log):
    from pytorch_sound_amd import kernels as K
    out, lin = K.mel_forward_nfk(mag, plan, M, log[0], log[1], None, log[2], log[3], want_lin=True)
    return lin, out


def run_backward(plan, K_, gout, lin, ref, log):
    """gmag of mel_backward_nfk (N, F, K), of mel_backward (N, K, F), gest of psnd_mel_l1_bwd_nfk (N, F, K)"""
    from pytorch_sound_amd import kernels as K
    g_nfk = K.mel_backward_nfk(gout, lin, plan, K_, log[0], log[1], None, log[2], log[3])
    g_nkf = K.mel_backward(gout, lin, plan, K_, log[0], log[1], None, log[2], log[3])
    return g_nfk, g_nkf, l1_bwd_nfk(ref, lin, plan, K_, log)


def same_bits(a, b, zeros_any_sign=False):
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape:
        return False
    if torch.equal(a.view(torch.int32), b.view(torch.int32)):
        return True
    if not zeros_any_sign:
        return False
    ne = a.view(torch.int32) != b.view(torch.int32)
    return bool(((a[ne] == 0) & (b[ne] == 0)).all())


_fix = {}


def fixture(name):
    if name not in _fix:
        d = {}
        for part in ('in', 'gmag', 'gest'):
            with np.load(os.path.join(GOLD, 'mel_bands_%s_%s.npz' % (name, part))) as z:
                d.update({k: z[k] for k in z.files})
        d['mag'] = from_bits16(d.pop('mag_bits16'))
        _fix[name] = {k: torch.from_numpy(v).to(DEV) for k, v in d.items()}
    return _fix[name]


_plans = {}


def plan_of(name):
    from pytorch_sound_amd import kernels as K
    if name not in _plans:
        _plans[name] = K.mel_plan(fixture(name)['W'].cpu().numpy()).to(DEV)
    return _plans[name]


@pytest.mark.parametrize('name,F_', [(n, f) for n, c in CASES.items() for f in c['Fs']])
def test_bits_against_recorded(name, F_):
    """lin / out of mel_forward_nfk, gmag of mel_backward_nfk and mel_backward, gest of psnd_mel_l1_bwd_nfk: the recorded bits"""
    fx, log = fixture(name), CASES[name]['log']
    M, K_ = fx['W'].shape
    plan = plan_of(name)
    dense = name in ('dense24', 'k17')          # a zero may change its sign where weights are negative (dropped acc + (+-0) steps)
    lin, out = run_forward(plan, M, fx['mag'][:, :F_].contiguous(), log)
    assert same_bits(lin, fx['lin'][:, :, :F_], dense), 'lin'
    assert same_bits(out, fx['out'][:, :, :F_], dense), 'out'
    cut = lambda k: fx[k][:, :, :F_].contiguous()   # noqa: E731
    g_nfk, g_nkf, gest = run_backward(plan, K_, cut('gout'), cut('lin'), cut('ref'), log)
    assert same_bits(g_nfk, fx['gmag'][:, :F_], dense), 'gmag (N, F, K)'
    assert same_bits(g_nkf, fx['gmag'][:, :F_].transpose(1, 2), dense), 'gmag (N, K, F)'
    assert same_bits(gest, fx['gest'][:, :F_], dense), 'gest'
    assert bool((gest != 0).any()) and bool((g_nfk != 0).any())


@pytest.mark.parametrize('name', ['slaney80', 'dense24'])
def test_regrouping(name):
    """a clip of F frames = its frames sent as F clips of one frame = clips of 16 and F - 16 frames, bit for bit"""
    fx, log = fixture(name), CASES[name]['log']
    M, K_ = fx['W'].shape
    plan = plan_of(name)
    F_ = CASES[name]['F']
    mag, gout, lin0, ref = fx['mag'][1:2].contiguous(), fx['gout'][1:2].contiguous(), fx['lin'][1:2].contiguous(), fx['ref'][1:2].contiguous()
    lin, out = run_forward(plan, M, mag, log)
    back = run_backward(plan, K_, gout, lin0, ref, log)
    back = (back[0], back[1].transpose(1, 2), back[2])               # all (1, F, K)
    # F clips of one frame
    lin1, out1 = run_forward(plan, M, mag.view(F_, 1, K_), log)
    assert same_bits(lin1[:, :, 0].t(), lin[0]) and same_bits(out1[:, :, 0].t(), out[0])
    as1 = lambda t: t[0].t().contiguous().view(F_, M, 1)             # noqa: E731  (1, M, F) -> (F, M, 1)
    b1 = run_backward(plan, K_, as1(gout), as1(lin0), as1(ref), log)
    for a, b in zip(back, (b1[0], b1[1].transpose(1, 2), b1[2])):
        assert same_bits(b.reshape(1, F_, K_), a)
    # clips of 16 and F - 16 frames
    for f0, f1 in ((0, 16), (16, F_)):
        lin2, out2 = run_forward(plan, M, mag[:, f0:f1].contiguous(), log)
        assert same_bits(lin2, lin[:, :, f0:f1]) and same_bits(out2, out[:, :, f0:f1])
        cut = lambda t: t[:, :, f0:f1].contiguous()                  # noqa: E731
        b2 = run_backward(plan, K_, cut(gout), cut(lin0), cut(ref), log)
        for a, b in zip(back, (b2[0], b2[1].transpose(1, 2), b2[2])):
            assert same_bits(b, a[:, f0:f1])


@pytest.mark.parametrize('F_', [17, 173])
def test_neighbours_do_not_leak(F_):
    """operands inside NaN-filled buffers (the frame behind the last one of a clip, the bins past K, the rows past the matrix) and outputs
    inside NaN-filled buffers: same bits, nothing written behind the output"""
    name = 'dense24'
    fx, log = fixture(name), CASES[name]['log']
    M, K_ = fx['W'].shape
    plan = plan_of(name)
    g = torch.Generator(device='cpu').manual_seed(F_)
    mag = torch.randn(2, F_, K_, generator=g).to(DEV)
    gout = torch.randn(2, M, F_, generator=g).to(DEV)
    ref = torch.randn(2, M, F_, generator=g).to(DEV)

    def padded(t):
        buf = torch.full((t.numel() + 256,), float('nan'), device=DEV)
        buf[128:128 + t.numel()] = t.flatten()
        return buf[128:128 + t.numel()].view(t.shape)

    from pytorch_sound_amd import kernels as K
    lin, out = run_forward(plan, M, mag, log)
    obuf = torch.full((out.numel() + 256,), float('nan'), device=DEV)
    out2, lin2 = K.mel_forward_nfk(padded(mag), plan, M, log[0], log[1], None, log[2], log[3], want_lin=True,
                                   out=obuf[128:128 + out.numel()].view(out.shape))
    assert same_bits(out2, out) and same_bits(lin2, lin)
    assert bool(torch.isnan(obuf[:128]).all()) and bool(torch.isnan(obuf[128 + out.numel():]).all())
    assert not bool(torch.isnan(out).any())
    a = run_backward(plan, K_, gout, lin, ref, log)
    b = run_backward(plan, K_, padded(gout), padded(lin), padded(ref), log)
    for x, y in zip(a, b):
        assert same_bits(x, y) and not bool(torch.isnan(x).any())


@pytest.mark.parametrize('N,F_', [(3, 17), (32, 173)])
def test_l1_partials(N, F_):
    """every partial sum of psnd_mel_l1_fwd_nfk is written by the launch; their float64 sum is the float64 value of
    sum |clip(log(W mag + 1e-6)) - ref| to 2e-6 (the tolerance of test_fused_spectral_l1_loss_nfk_equals_nkf)"""
    from pytorch_sound_amd._lib import lib
    name = 'slaney80'
    log = CASES[name]['log']
    W = fixture(name)['W']
    M, K_ = W.shape
    plan = plan_of(name)
    g = torch.Generator(device='cpu').manual_seed(N * F_)
    mag = (torch.rand(N, F_, K_, generator=g) * 4).to(DEV)
    mag[0, 0] = 0
    ref = (torch.randn(N, M, F_, generator=g) * 2).to(DEV)
    # the count of the (N, F, K) forward is still that of the (N, K, F) one: one partial per (clip, 64 frames, 16 mel bands)
    nb = int(lib().psnd_mel_l1_blocks(N, F_, M))
    assert nb == N * ((F_ + 63) // 64) * ((M + 15) // 16)
    part = torch.full((nb + 8,), float('nan'), dtype=torch.float64, device=DEV)
    lin = l1_fwd_nfk(mag, ref, plan, M, log, part)
    assert bool(torch.isfinite(part[:nb]).all()) and bool(torch.isnan(part[nb:]).all())
    lin0, _ = run_forward(plan, M, mag, log)
    assert same_bits(lin, lin0)
    y = torch.clamp(torch.log(torch.einsum('mk,nfk->nmf', W.double(), mag.double()) + 1e-6), log[2], log[3])
    want = float((y - ref.double()).abs().sum())
    got = float(part[:nb].sum())
    assert abs(got - want) <= 2e-6 * abs(want), (got, want)
