"""No HIP path may depend on what freed device memory last held.

The host code takes ~140 buffers from torch.empty / empty_like and trusts the kernels to write every halo row, padded channel, slab
entry and partial-tile row that is read later.  Every case here runs one product path forward and backward on fixed seeded inputs with
the allocator's free blocks filled with 0x00, 0xFF (NaN / -1) and 0x7F (3.4e38, finite: it survives the max() and comparisons that
swallow a NaN) - tests/poison.py, which also asserts that the poison reached torch.empty and that the run was served from poisoned
memory alone.  The inputs are identical, so for the paths that add in fixed orders the three results must be the SAME BITS and finite:
no tolerance.  psnd_stft_bwd* adds with atomics outside its plain-store interior: the waveform gradients that end in it are compared
with the float64 oracle on every pattern, at the tolerance of the existing test of that path (test_stft_bwd_vs_oracle: 5e-5 through the
magnitude; smoke(): 2e-4 through the log-mel; test_multi_stft_loss_vs_oracle: gtol 2e-4 at eps 1e-2); their forward outputs bit for bit.

Poison read as a value gives a wrong number; read as an index it could send a kernel out of bounds.  The integer- and pointer-typed
device buffers on these paths are all written in full by the host before a kernel reads them: the descriptor tables of cl.prep_all /
prep_all_convtr (bytes joined on the host, one .to(device)), the STFT and mel plans (numpy -> torch -> .to(device)), the Adam table
(packed on the host into a pinned buffer, copied whole) with its chunk_tensor / chunk_off (numpy, .to(device)), the key masks (made by the
caller), the wgrad_multi descriptors and the loss block counts (host arrays read during the call).  The kernels keep counters and locks
in LDS only; the library allocates no device memory of its own.

The private pool of a captured graph and the two-GPU paths are out of reach of this method (test_gpu_trainer_graph.py compares replay
with eager)."""
import ctypes
import os
import sys
import tempfile
import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison as P  # noqa: E402
from conftest import seeded_wav  # noqa: E402
from oracle import features as ofe  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _grads(mod):
    return {k: p.grad for k, p in mod.named_parameters()}


def _zero(*mods):
    for m in mods:
        for p in m.parameters():
            p.grad = None


def _check_loose(results, name, ref, tol):
    """the results that end in psnd_stft_bwd's atomics: finite and equal to the float64 oracle on every pattern"""
    for byte, r in zip(P.PATTERNS, results):
        got = r['loose'][name].double().numpy()
        assert np.isfinite(got).all(), '%s is not finite on pattern 0x%02X' % (name, byte)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= tol, '%s on pattern 0x%02X: %.3g of max against the float64 oracle (bound %.3g)' % (name, byte, err, tol)


def _bits_and_loose(fn):
    """fn() -> {'bits': ..., 'loose': {...}}: the 'bits' part must not depend on the pattern; the 'loose' part is returned for _check_loose"""
    results = P.run_on_patterns(fn)
    bits = [r['bits'] for r in results]
    bad = P.not_finite(bits) + P.differences(bits)
    assert not bad, 'the path reads memory it did not write:\n  ' + '\n  '.join(bad[:20])
    return results


# ---- the helper itself -------------------------------------------------------------------------------------------------------------------
def test_helper_reports_a_read_of_unwritten_memory_and_nothing_else():
    """no product code: a function that writes the even elements of a torch.empty buffer and sums the odd ones depends on the pattern; the
    same on torch.zeros does not.  Values only - nothing uninitialised is used as an address."""
    n = 100001

    def make(alloc):
        def fn():
            buf = alloc(n, dtype=torch.float32, device=DEV)
            buf[0::2] = 1.0
            return [buf[1::2].sum(), buf[0::2].sum()]
        return fn

    results = P.run_on_patterns(make(torch.empty))
    assert [float(r[0]) for r in results][0] == 0.0
    assert float(results[1][0]) > 1e38 and np.isnan(float(results[2][0]))        # 0x7F: 50000 x 3.39e38 -> inf; 0xFF: NaN
    diff, nf = P.differences(results), P.not_finite(results)
    assert len(diff) == 2 and all(d.startswith('r[0] ') for d in diff), diff        # the odd sum on both poisoned patterns, never the even sum
    assert len(nf) == 2, nf
    with pytest.raises(AssertionError, match='reads memory it did not write'):
        P.assert_same_bits(make(torch.empty))
    for run in P.LAST['runs']:
        assert run['blocks'] >= 1 and run['bytes'] >= 4 * n and run['reserved_before'] == run['reserved_after']
    P.assert_same_bits(make(torch.zeros))


# ---- channels-last conv family -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Cin,Cout,k,dil,L,N,role', [(513, 256, 3, 1, 173, 2, 'both'), (64, 40, 7, 3, 61, 2, 'both'), (32, 32, 11, 5, 8192, 8, 'both'),
                                                    (80, 512, 7, 1, 32, 16, 'act'), (64, 64, 3, 1, 50, 2, 'raw'), (128, 128, 11, 5, 64, 2, 'act')])
def test_fused_conv(Cin, Cout, k, dil, L, N, role):
    """cl.fused_conv (psnd_conv1d_cl, _bwd, _wgrad, _wnorm_bwd, psnd_to_cl / psnd_from_cl) with the residual and both outputs, and in the head
    ('act' only) / tail ('raw' only) roles of a chain; shapes of test_fused_conv_fwd_bwd / test_single_output_conv_exact_on_rounded_operands"""
    from pytorch_sound_amd import cl
    from pytorch_sound_amd.models.vocoders.hifi_gan import WNConv1d
    torch.manual_seed(Cin + k)
    pad = (k * dil - dil) // 2
    conv = WNConv1d(Cin, Cout, k, dil, pad, init_std=0.05).to(DEV)
    x, r = torch.randn(N, Cin, L, device=DEV), torch.randn(N, Cout, L, device=DEV)
    gy, gya = torch.randn(N, Cout, L, device=DEV), torch.randn(N, Cout, L, device=DEV)

    def fn():
        _zero(conv)
        shape = cl.CLShape(N, L, pad + 1)
        xc, rc = x.clone().requires_grad_(True), r.clone().requires_grad_(True)
        xb = cl.ToCL.apply(xc, shape, 0)
        if role == 'both':
            yb, yab = cl.fused_conv(xb, conv, shape, cl.ToCL.apply(rc, shape, 0), True, True, 0.1)
            y2, ya2 = cl.FromCL.apply(yb, Cout, L, shape), cl.FromCL.apply(yab, Cout, L, shape)
            ((y2 * gy).sum() + (ya2 * gya).sum()).backward()
            return [yb, yab, y2, ya2, xc.grad, rc.grad, _grads(conv)]        # yb / yab whole: halo rows and padded channels included
        yb, yab = cl.fused_conv(xb, conv, shape, None, role == 'raw', role == 'act', 0.1)
        buf = yab if role == 'act' else yb
        out = cl.FromCL.apply(buf, Cout, L, shape)
        (out * gy).sum().backward()
        return [buf, out, xc.grad, _grads(conv)]

    P.assert_same_bits(fn)


@pytest.mark.parametrize('Cin,Cout,u,L,N,hp_in,hp_out,covers', [(128, 64, 4, 61, 2, 3, 11, True),
                                                                # the low rows do not reach row 0 of the output: cl._up_covers is false, the outputs are zeroed first
                                                                (16, 8, 2, 24, 1, 3, 11, False), (128, 64, 4, 61, 2, 3, 25, False)])
def test_conv_transpose_cl(Cin, Cout, u, L, N, hp_in, hp_out, covers):
    """cl.ConvTransposeCL (psnd_convtr1d_prep, _cl_fwd, _cl_bwd, _cl_wgrad, psnd_cl_colsum): both outputs whole, input and parameter gradients"""
    from pytorch_sound_amd import cl
    from pytorch_sound_amd.models.vocoders.hifi_gan import WNConvTranspose1d
    torch.manual_seed(Cin + u)
    pad = u // 2
    up = WNConvTranspose1d(Cin, Cout, 2 * u, u, pad, init_std=0.05).to(DEV)
    x = torch.randn(N, Cin, L, device=DEV)
    gy, gya = torch.randn(N, Cout, L * u, device=DEV), torch.randn(N, Cout, L * u, device=DEV)
    shape, out_shape = cl.CLShape(N, L, hp_in), cl.CLShape(N, L * u, hp_out)
    assert cl._up_covers(shape, out_shape, u, pad) == covers

    def fn():
        _zero(up)
        xc = x.clone().requires_grad_(True)
        raw, act = cl.ConvTransposeCL.apply(cl.ToCL.apply(xc, shape, 0), up.weight_v, up.weight_g, up.bias, shape, out_shape, u, pad, 0.1)
        y2, ya2 = cl.FromCL.apply(raw, Cout, L * u, out_shape), cl.FromCL.apply(act, Cout, L * u, out_shape)
        ((y2 * gy).sum() + (ya2 * gya).sum()).backward()
        torch.cuda.synchronize()                                      # the parameter side runs on its own stream
        return [raw, act, y2, ya2, xc.grad, _grads(up)]

    P.assert_same_bits(fn)


def test_layout_kernels():
    """ToCL (plain and log1p) / FromCL / to_cl_nfk / FromCLTanh with their backward passes, ragged channel counts (513, 1) and lengths"""
    from pytorch_sound_amd import cl
    torch.manual_seed(3)
    N, C, T = 3, 513, 173
    shape = cl.CLShape(N, T, 25)
    x = torch.rand(N, C, T, device=DEV) * 4
    x_nfk = x.transpose(1, 2).contiguous()
    g = torch.randn(N, C, T, device=DEV)
    one = torch.randn(N, 1, T, device=DEV)

    def fn():
        out = []
        for preop in (0, 1):
            xc = x.clone().requires_grad_(True)
            b = cl.ToCL.apply(xc, shape, preop)
            y = cl.FromCL.apply(b, C, T, shape)
            (y * g).sum().backward()
            out += [b, y, xc.grad, cl.to_cl_nfk(x_nfk, shape, preop)]
        oc = one.clone().requires_grad_(True)
        t = cl.FromCLTanh.apply(cl.ToCL.apply(oc, shape, 0), 1, T, shape)
        (t * g[:, :1]).sum().backward()
        return out + [t, oc.grad]

    P.assert_same_bits(fn)


# ---- whole models ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,launches', [(8, 'chain'), (8, 'pair'), (32, 'chain'), (32, 'pair')])
def test_separator(N, launches, monkeypatch, capsys):
    """conv_separator_voicebank (256 channels, 4 blocks) on N x 513 x 173, the launch modes of test_separator_bench_shape_vs_bf16_emulation:
    the mask-head path without an input gradient (what the bench runs) and the path with one; output, input gradient, all parameter gradients"""
    from pytorch_sound_amd.models import build_model
    from pytorch_sound_amd.models import separator  # noqa: F401
    if launches == 'pair':
        monkeypatch.setenv('PSND_CL_CHAIN', '0')
        monkeypatch.setenv('PSND_CL_BWD_BATCH', '0')
    torch.manual_seed(2024)
    model = build_model('conv_separator_voicebank').to(DEV)
    mag, tgt = torch.rand(N, 513, 173, device=DEV) * 4, torch.rand(N, 513, 173, device=DEV) * 4

    def fn():
        out = []
        for need_gx in (False, True):
            _zero(model)
            m = mag.clone().requires_grad_(need_gx)
            est = model(m)
            F.l1_loss(est, tgt).backward()
            torch.cuda.synchronize()
            out += [est, m.grad, _grads(model)]
        return out

    r = P.assert_same_bits(fn)
    assert len(r[2]) > 50
    with capsys.disabled():
        print('\n[poison] separator N=%d %s: %s' % (N, launches, P.LAST['runs']))


@pytest.mark.parametrize('N,T,channels', [(32, 173, 256), (3, 61, 64)])
def test_separator_fused_spectral_l1_loss(N, T, channels):
    """ConvSeparator.spectral_l1_loss (mask head + both L1 terms as one node: block partials in double, psnd_mel_l1_fwd's linear mel)"""
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd.models import build_model
    from pytorch_sound_amd.models import separator  # noqa: F401
    from pytorch_sound_amd.models.transforms import LogMelSpectrogram
    torch.manual_seed(7 + T)
    model = build_model('conv_separator_voicebank', {'channels': channels, 'num_blocks': 2}).to(DEV)
    fe = LogMelSpectrogram(22050, 80, 1024, 1024, 256, -50, 30, 0.0, 8000.0).to(DEV)
    mag, mag_ref = torch.rand(N, 513, T, device=DEV) * 4, torch.rand(N, 513, T, device=DEV) * 4
    mel_ref = K.MelLog.apply(mag_ref, fe._mel_plan(), 80, K.LOG_E, 1e-6, None, fe.min_db, fe.max_db)

    def fn():
        _zero(model)
        loss, est = model.spectral_l1_loss(mag, mag_ref, mel_ref, fe._mel_plan(), 80, 1.0, 0.5, 1e-6, fe.min_db, fe.max_db)
        loss.backward()
        torch.cuda.synchronize()
        return [loss, est, _grads(model)]

    P.assert_same_bits(fn)


def _tiny_generator(resblock, rates, ksz, c0, rk, rd):
    from argparse import Namespace
    from pytorch_sound_amd.models.vocoders.hifi_gan import Generator
    torch.manual_seed(5)
    h = Namespace(resblock=resblock, upsample_rates=rates, upsample_kernel_sizes=ksz, upsample_initial_channel=c0,
                  resblock_kernel_sizes=rk, resblock_dilation_sizes=rd)
    g = Generator(h).to(DEV)
    with torch.no_grad():
        for n, p in g.named_parameters():
            if n.endswith('weight_v'):
                p.mul_(10.0 if p.abs().max() < 0.1 else 1.0)
    return g


TINY = {'v1': ('1', [4, 2], [8, 4], 64, [3, 7, 11], [[1, 3, 5], [1, 3, 5], [1, 3, 5]]),
        'v2': ('2', [4, 4], [8, 8], 64, [3, 5], [[1, 2], [2, 6]]),
        'v3': ('2', [8, 4], [16, 8], 32, [3, 7], [[1, 2], [2, 6]])}


def _generator_case(g, x, w):
    def fn():
        _zero(g)
        xc = x.clone().requires_grad_(True)
        out = g(xc)
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return [out, xc.grad, _grads(g)]
    P.assert_same_bits(fn)


@pytest.mark.parametrize('cfg', sorted(TINY))
@pytest.mark.parametrize('upsample', ['polyphase', 'kernel'])
def test_hifi_gan_tiny_bf16(cfg, upsample):
    """tiny HiFi-GAN generators (ResBlock1 / ResBlock2, the configs of test_generator_cl_matches_torch_path and a v3-like one with stride 8)
    on the channels-last bf16 kernels: output, input gradient, every parameter gradient"""
    g = _tiny_generator(*TINY[cfg])
    g.cl_upsample = upsample
    x = torch.randn(3, 80, 24, device=DEV)
    assert g._cl_ok(x)
    _generator_case(g, x, torch.randn(3, 1, 24 * int(np.prod(TINY[cfg][1])), device=DEV))


@pytest.mark.parametrize('arch,shape', [('hifi_gan_v1', (4, 80, 32)), ('hifi_gan_v2', (2, 80, 24)), ('hifi_gan_v3', (2, 80, 24))])
def test_hifi_gan_registered_bf16(arch, shape):
    from pytorch_sound_amd.models import build_model
    from pytorch_sound_amd.models.vocoders import hifi_gan  # noqa: F401
    torch.manual_seed(2)
    g = build_model(arch).to(DEV)
    x = torch.randn(*shape, device=DEV)
    with torch.no_grad():
        T_out = g(x).shape[-1]
    _generator_case(g, x, torch.randn(shape[0], 1, T_out, device=DEV))


@pytest.mark.native_precision
@pytest.mark.parametrize('cfg', ['v1', 'v2'])
def test_hifi_gan_tiny_fp32_im2col(cfg):
    """the fp32 instance (psnd_im2col_f32 / psnd_col2im_f32 around fp32 products): what an fp32 HIP tensor outside autocast gets"""
    g = _tiny_generator(*TINY[cfg])
    x = torch.randn(3, 80, 24, device=DEV)
    _generator_case(g, x, torch.randn(3, 1, 24 * int(np.prod(TINY[cfg][1])), device=DEV))


# ---- transformer block -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,H,C,T,masked', [(8, 4, 256, 173, True), (2, 2, 96, 77, False)])
@pytest.mark.parametrize('autocast', [False, True])
def test_transformer_block(N, H, C, T, masked, autocast):
    """1x1 projection -> PositionalEncoding -> MultiHeadAttention -> PointwiseFeedForward -> 1x1 projection (the config-4 block; psnd_linear1x1_*,
    psnd_posenc, psnd_mha_*, psnd_groupnorm1_*), fp32 and bf16 forms, the attention tensor returned and in the loss in the fp32 form"""
    from pytorch_sound_amd.models import modules as M
    torch.manual_seed(T)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inp, self.pe = torch.nn.Conv1d(80, C, 1), M.PositionalEncoding(C, 512)
            self.mha, self.ffn, self.out = M.MultiHeadAttention(C, H, 0.0), M.PointwiseFeedForward(C, 0.0), torch.nn.Conv1d(C, 80, 1)
            self.mha.return_att = not autocast

        def forward(self, x, pad):
            y, att = self.mha(self.pe(M._conv1x1(self.inp, x)), pad)
            return M._conv1x1(self.out, self.ffn(y)), att

    net = Net().to(DEV)
    lens = torch.linspace(T, max(T // 3, 8), N).long()
    pad = (torch.arange(T)[None, :] >= lens[:, None]).to(DEV) if masked else None
    x = 0.1 * torch.randn(N, 80, T, device=DEV)
    w, gatt = torch.randn(N, 80, T, device=DEV), 0.1 * torch.randn(H * N, T, T, device=DEV)

    def fn():
        _zero(net)
        xc = x.clone().requires_grad_(True)
        with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
            y, att = net(xc, pad)
        loss = (y.float() * w).sum()
        if not autocast:
            loss = loss + (att * gatt).sum()
        loss.backward()
        torch.cuda.synchronize()
        return [y, att if not autocast else None, xc.grad, _grads(net)]

    P.assert_same_bits(fn)


def test_softmax_keys_and_posenc():
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd.models import modules as M
    torch.manual_seed(1)
    B, T = 5, 173
    s = torch.randn(B, T, T, device=DEV) * 3
    mask = torch.zeros(B, T, dtype=torch.bool, device=DEV)
    for i, L in enumerate([173, 100, 64, 173, 9]):
        mask[i, L:] = True
    ga = torch.randn(B, T, T, device=DEV)
    pe = M.PositionalEncoding(30, 1200).to(DEV)
    xp, gp = torch.randn(3, 30, 1000, device=DEV), torch.randn(3, 30, 1000, device=DEV)

    def fn():
        sx = s.clone().requires_grad_(True)
        att = K.SoftmaxKeys.apply(sx, mask.to(torch.uint8), 1.0 / 8.0)
        (att * ga).sum().backward()
        xc = xp.clone().requires_grad_(True)
        y = pe(xc)
        y.backward(gp)
        return [att, sx.grad, y, xc.grad]

    P.assert_same_bits(fn)


@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('bf16', [False, True])
def test_linear1x1(relu, bf16):
    from pytorch_sound_amd import kernels as K
    torch.manual_seed(3173)
    N, Cin, Cout, T = 3, 80, 256, 173
    x, b, g = torch.randn(N, Cin, T, device=DEV), torch.randn(Cout, device=DEV), torch.randn(N, Cout, T, device=DEV)
    w = torch.randn(Cout, Cin, 1, device=DEV) / Cin ** 0.5

    def fn():
        xc, wc, bc = (t.clone().requires_grad_(True) for t in (x, w, b))
        y = K.Linear1x1.apply(xc, wc, bc, relu, bf16)
        (y * g).sum().backward()
        return [y, xc.grad, wc.grad, bc.grad]

    P.assert_same_bits(fn)


def test_relu_link_between_two_projections():
    """PointwiseFeedForward alone (Conv1d -> ReLU -> Conv1d -> GroupNorm with the residual): the ReLU link of psnd_linear1x1_bwd_ex, fp32
    and with the hidden tensor stored as bf16 under autocast"""
    from pytorch_sound_amd.models import modules as M
    torch.manual_seed(4)
    ffn = M.PointwiseFeedForward(256, 0.0).to(DEV)
    x, g = torch.randn(3, 256, 173, device=DEV), torch.randn(3, 256, 173, device=DEV)

    def fn():
        out = []
        for ac in (False, True):
            _zero(ffn)
            xc = x.clone().requires_grad_(True)
            with torch.autocast('cuda', dtype=torch.bfloat16, enabled=ac):
                y = ffn(xc)
            (y.float() * g).sum().backward()
            torch.cuda.synchronize()
            out += [y, xc.grad, _grads(ffn)]
        return out

    P.assert_same_bits(fn)


# ---- features ----------------------------------------------------------------------------------------------------------------------------
STFT_GEOMETRIES = [(256, 64, 2, 700), (512, 128, 40, 2600), (512, 129, 2, 3000), (1024, 256, 4, 44100), (1024, 255, 2, 2049), (2048, 512, 3, 20000),
                   (2048, 600, 1, 20000), (4096, 1024, 3, 44100), (4096, 1023, 1, 20000), (128, 32, 2, 500)]


@pytest.mark.parametrize('n_fft,hop,N,T', STFT_GEOMETRIES)
def test_stft_transform(n_fft, hop, N, T):
    """STFT.transform with a waveform gradient, one geometry per forward kernel: magnitude and phase bit for bit, the gradient (psnd_stft_bwd)
    against the float64 oracle on every pattern (5e-5 of max, test_stft_bwd_vs_oracle)"""
    from pytorch_sound_amd.models.transforms import STFT
    m = STFT(n_fft, hop).to(DEV)
    wav_np = seeded_wav(n_fft + hop + T, N, T)
    wav = torch.from_numpy(wav_np).to(DEV)
    Fr = ofe.frame_count(T, n_fft, hop, 0)
    gmag_np = np.random.RandomState(T).randn(N, n_fft // 2 + 1, Fr).astype(np.float32)
    gmag = torch.from_numpy(gmag_np).to(DEV)

    def fn():
        x = wav.clone().requires_grad_(True)
        mag, phase = m.transform(x)
        (mag * gmag).sum().backward()
        return {'bits': [mag, phase], 'loose': {'gwav': x.grad}}

    results = _bits_and_loose(fn)
    _check_loose(results, 'gwav', ofe.stft_mag_bwd_f64(gmag_np, wav_np, n_fft, hop, None, 0), 5e-5)


def test_stft_dense_basis_800():
    """filter_length 800 / hop 200: the dense-basis products of dense.py (forward)"""
    from pytorch_sound_amd.models.transforms import STFT
    m = STFT(800, 200).to(DEV)
    wav = torch.from_numpy(seeded_wav(800, 2, 5000)).to(DEV)

    def fn():
        with torch.no_grad():
            mag, phase = m.transform(wav)
            return [mag, phase, m.inverse(mag, phase)]

    P.assert_same_bits(fn)


@pytest.mark.parametrize('n_fft,hop,N,T', [(1024, 256, 4, 44100), (1024, 250, 2, 6000), (1024, 512, 2, 9000), (4096, 1024, 3, 44100), (4096, 1022, 1, 20000),
                                           (4096, 1024, 21, 60000), (512, 128, 2, 3000), (2048, 512, 2, 9000)])
def test_stft_nfk_kernels(n_fft, hop, N, T):
    """the bin-fastest (N, F, K) magnitude kernels: four frames per wave (1024), the ring (4096, hop 1024) and register-load (4096) kernels, one
    frame per workgroup elsewhere"""
    from pytorch_sound_amd import kernels as K
    plan = K.stft_plan(n_fft, ofe.analysis_window(n_fft)).to(DEV)
    wav = torch.from_numpy(seeded_wav(n_fft + T, N, T)).to(DEV)
    P.assert_same_bits(lambda: [K.stft_mag_nfk(wav, n_fft, hop, plan, 0, 0.0)])


@pytest.mark.parametrize('N,T,hop,M,fused', [(3, 44100, 256, 80, True), (1, 5000, 200, 40, True), (2, 6000, 300, 80, False)])
def test_logmel(N, T, hop, M, fused):
    """LogMelSpectrogram on the fused kernel and on the two-kernel path (a hop the fused kernel does not take), forward bit for bit, the
    waveform gradient against the float64 oracle on every pattern (2e-4 of max: the bound of smoke())"""
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd.models.transforms import LogMelSpectrogram
    fe = LogMelSpectrogram(22050, M, 1024, 1024, hop, -50, 30, 0, 8000).to(DEV)
    wav_np = seeded_wav(T + hop, N, T)
    wav = torch.from_numpy(wav_np).to(DEV)
    assert bool(K.logmel_fused_ok(wav, 1024, hop)) == fused
    Fr = ofe.frame_count(T, 1024, hop, 0)
    g_np = np.random.RandomState(M).randn(N, M, Fr).astype(np.float32)
    g = torch.from_numpy(g_np).to(DEV)

    def fn():
        with torch.no_grad():
            mel_nograd = fe(wav)                    # the fused kernel where it applies (forward only)
        x = wav.clone().requires_grad_(True)
        mel = fe(x)                                 # STFT magnitude + psnd_mel_fwd, the backward through psnd_mel_bwd and psnd_stft_bwd
        (mel * g).sum().backward()
        return {'bits': [mel_nograd, mel], 'loose': {'gwav': x.grad}}

    results = _bits_and_loose(fn)
    W = ofe.mel_filterbank(22050, 1024, M, 0, 8000).astype(np.float64)
    mag = ofe.stft_mag_f64(wav_np, 1024, hop)
    lin = W @ mag + 1e-6
    y = np.log(lin)
    lo, hi = ofe.db_to_ln(-50), ofe.db_to_ln(30)
    gmag = np.einsum('mk,nmf->nkf', W, g_np * np.where((y < lo) | (y > hi), 0.0, 1.0 / lin))
    _check_loose(results, 'gwav', ofe.stft_mag_bwd_f64(gmag, wav_np, 1024, hop), 2e-4)


def test_mel_log_forward_and_backward():
    """K.MelLog on a magnitude leaf (psnd_mel_fwd / _bwd: no STFT adjoint behind it), F = 173 and a ragged mel count"""
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd.models.transforms import LogMelSpectrogram
    fe = LogMelSpectrogram(16000, 40, 512, 512, 128, -50, 30, 50, 7000).to(DEV)
    torch.manual_seed(6)
    mag, g = torch.rand(3, 257, 173, device=DEV) * 4, torch.randn(3, 40, 173, device=DEV)

    def fn():
        m = mag.clone().requires_grad_(True)
        y = K.MelLog.apply(m, fe._mel_plan(), 40, K.LOG_E, 1e-6, None, fe.min_db, fe.max_db)
        (y * g).sum().backward()
        return [y, m.grad]

    P.assert_same_bits(fn)


@pytest.mark.parametrize('kind', ['STFT', 'STFTTorchAudio'])
def test_istft_with_gradients_to_magnitude_and_phase(kind):
    from pytorch_sound_amd.models import transforms as TR
    n_fft, hop, Fr = 1024, 256, 21
    m = getattr(TR, kind)(n_fft, hop).to(DEV)
    rs = np.random.RandomState(1)
    mag = torch.from_numpy((np.abs(rs.randn(2, 513, Fr)) + 0.1).astype(np.float32)).to(DEV)
    phase = torch.from_numpy(rs.uniform(-3, 3, (2, 513, Fr)).astype(np.float32)).to(DEV)
    gout = torch.from_numpy(rs.randn(2, (Fr - 1) * hop).astype(np.float32)).to(DEV)

    def fn():
        mt, pt = mag.clone().requires_grad_(True), phase.clone().requires_grad_(True)
        out = m.inverse(mt, pt)
        (out * gout).sum().backward()
        return [out, mt.grad, pt.grad]

    P.assert_same_bits(fn)


@pytest.mark.parametrize('n,hop,N,T', [(150, 37, 3, 1999), (1024, 256, 8, 32000)])
def test_learnable_stft(n, hop, N, T):
    """LearnableSTFT transform + inverse + both basis gradients (psnd_lstft_*: slab sums, bit-stable - test_same_bits_from_run_to_run)"""
    from pytorch_sound_amd.models.transforms import LearnableSTFT
    m = LearnableSTFT(n, hop)
    gen = torch.Generator().manual_seed(0)
    with torch.no_grad():
        m.forward_basis.add_(0.05 * torch.randn(m.forward_basis.shape, generator=gen))
        m.inverse_basis.add_(0.05 / n * torch.randn(m.inverse_basis.shape, generator=gen))
    m = m.to(DEV)
    wav = torch.from_numpy(seeded_wav(n + T, N, T)).to(DEV)

    def fn():
        _zero(m)
        x = wav.clone().requires_grad_(True)
        mag, phase = m.transform(x)
        rec = m.inverse(mag, phase)
        (mag.sum() + rec.pow(2).sum()).backward()
        torch.cuda.synchronize()
        return [mag, phase, rec, x.grad, _grads(m)]

    P.assert_same_bits(fn)


def test_pqmf_and_preemphasis():
    """PQMF analysis / synthesis at 8 bands, 126 taps, a length that is no multiple of anything, and PreEmphasis; forward and backward"""
    from pytorch_sound_amd.models.transforms import PQMF
    from pytorch_sound_amd.models.sound import PreEmphasis
    pq = PQMF(subbands=8, taps=126, cutoff_ratio=0.07, beta=10.0).to(DEV)
    pe = PreEmphasis(0.97).to(DEV)
    x = torch.from_numpy(np.random.RandomState(5).randn(2, 1, 8192 + 8).astype(np.float32)).to(DEV)
    xo = torch.from_numpy(np.random.RandomState(6).randn(3, 1, 4099).astype(np.float32)).to(DEV)

    def fn():
        xc = x.clone().requires_grad_(True)
        a = pq.analysis(xc)
        y = pq.synthesis(a)
        (y.pow(2).sum() + a.sum()).backward()
        xe = xo.clone().requires_grad_(True)
        e = pe(xe)
        e.pow(2).sum().backward()
        return [a, y, xc.grad, e, xe.grad]

    P.assert_same_bits(fn)


# ---- losses ------------------------------------------------------------------------------------------------------------------------------
def test_l1_losses():
    """l1_loss at (1, 16385) and (5,), l1_loss_sum, masked_l1_loss at (3, 5, 7): double partials per block, summed by a second kernel"""
    from pytorch_sound_amd import kernels as K
    torch.manual_seed(5)
    pairs = [(torch.randn(*s, device=DEV), torch.randn(*s, device=DEV)) for s in ((1, 16385), (5,), (3, 513, 173), (3, 80, 173), (3, 5, 7))]
    wgt = (torch.arange(7)[None, :] < torch.tensor([7, 3, 1])[:, None]).float().to(DEV)

    def fn():
        out = []
        leaf = [(a.clone().requires_grad_(True), b.clone().requires_grad_(True)) for a, b in pairs]
        for a, b in leaf[:2]:
            loss = K.l1_loss(a, b)
            (3.0 * loss).backward()
            out += [loss, a.grad, b.grad]
        loss = K.l1_loss_sum([leaf[2], leaf[3]], (1.0, 0.5))
        (2.0 * loss).backward()
        out += [loss, leaf[2][0].grad, leaf[2][1].grad, leaf[3][0].grad, leaf[3][1].grad]
        loss = K.masked_l1_loss(leaf[4][0], leaf[4][1], wgt)
        (1.7 * loss).backward()
        return out + [loss, leaf[4][0].grad, leaf[4][1].grad]

    P.assert_same_bits(fn)


@pytest.mark.parametrize('fused', ['1', '0'])
@pytest.mark.parametrize('N,T', [(2, 3001), (16, 8192)])
def test_multi_stft_loss(N, T, fused, monkeypatch):
    """multi_stft_loss, training case (the prediction alone needs a gradient) on the fused kernels (psnd_stft_fwd_msl / psnd_stft_bwd_msl) and
    on the separate ones: the three loss values bit for bit, the gradient against the float64 oracle on every pattern (eps 1e-2: gtol 2e-4)"""
    from oracle import sound as osnd
    from pytorch_sound_amd.models.sound import multi_stft_loss, build_stft_functions
    from pytorch_sound_amd.models.transforms import centre_pad
    PARAMS, eps, gtol = [(1024, 600, 120), (2048, 1200, 240), (512, 240, 50)], 1e-2, 2e-4
    monkeypatch.setenv('PSND_MSL_FUSED', fused)
    t = seeded_wav(900 + N, N, T)
    p = (0.8 * t + 0.05 * seeded_wav(950 + N, N, T)).astype(np.float32)
    target, pred0 = torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV)

    def fn():
        pred = pred0.clone().requires_grad_(True)
        loss, sc, mag = multi_stft_loss(pred, target, PARAMS, eps)
        (0.5 * loss + 2.0 * sc - 0.25 * mag).backward()
        return {'bits': [loss, sc, mag], 'loose': {'gpred': pred.grad}}

    results = _bits_and_loose(fn)
    wins = [centre_pad(f.window.numpy().astype(np.float64), f.n_fft) for f in build_stft_functions(*PARAMS)]
    gp = np.zeros_like(p, dtype=np.float64)
    for (n_fft, win, hop), w in zip(PARAMS, wins):
        pm = osnd.stft_mag_torchaudio_f64(p, n_fft, win, hop, w)
        tm = osnd.stft_mag_torchaudio_f64(t, n_fft, win, hop, w)
        a, _ = osnd.stft_loss_terms_bwd(pm, tm, (0.5 + 2.0) / 3, (0.5 - 0.25) / 3, eps)
        gp += ofe.stft_mag_bwd_f64(a, p, n_fft, hop, framing=ofe.CENTER, window=w)
    _check_loose(results, 'gpred', gp, gtol)


# ---- optimizer and step ------------------------------------------------------------------------------------------------------------------
def test_three_trainer_steps_with_hip_adam_and_clip_by_norm():
    """three eager Trainer steps of the small separator with pytorch_sound_amd.optim.Adam and grad_norm on (psnd_grad_sumsq, psnd_adam_step),
    the free memory poisoned before every step: parameters and Adam state after step 3 are the same bits on all patterns"""
    from pytorch_sound_amd.models import build_model
    from pytorch_sound_amd.models import separator  # noqa: F401
    from pytorch_sound_amd.models.transforms import STFT
    from pytorch_sound_amd.optim import Adam
    from pytorch_sound_amd.trainer import Trainer, LogType
    stft = STFT(1024, 256).to(DEV)
    wavs = [(torch.from_numpy(seeded_wav(10 + i, 2, 6000)).to(DEV), torch.from_numpy(0.5 * seeded_wav(20 + i, 2, 6000)).to(DEV)) for i in range(3)]

    class Step(Trainer):
        def forward(self, noisy, clean, is_logging=False):
            est = self.model(stft.magnitude(noisy))
            with torch.no_grad():
                tgt = stft.magnitude(clean)
            loss = F.l1_loss(est, tgt)
            return loss, {'loss': (loss, LogType.SCALAR)}

    def fn(repoison):
        torch.manual_seed(1)
        model = build_model('conv_separator_voicebank', {'channels': 32, 'num_blocks': 1}).to(DEV)
        opt = Adam(model.parameters(), lr=1e-3)
        tr = Step(model, opt, wavs, wavs[:1], max_step=10 ** 9, valid_max_step=1, save_interval=10 ** 9, log_interval=10 ** 9,
                  save_dir=tempfile.mkdtemp(prefix='psnd_poison_'), grad_norm=0.5, seed=1)
        tr.graph_steps = False
        model.train()
        for i in range(1, 4):
            repoison()
            tr.step = i
            tr.train(i)
        torch.cuda.synchronize()
        state = [[opt.state[p][k] for k in ('step', 'exp_avg', 'exp_avg_sq')] for p in model.parameters()]
        return [dict(model.state_dict()), state]

    r = P.assert_same_bits(fn)
    assert all(float(s[0]) == 3.0 for s in r[1])


def _fill(t, byte):
    t.reshape(-1).view(torch.uint8).fill_(byte)
    return t


def _on_prefilled(call, shapes, patterns=(0x00, 0xFF)):
    """a C ABI call on caller-owned buffers: `call(bufs)` with every buffer of `shapes` {name: (shape, dtype)} pre-filled with the pattern's
    byte - outputs AND workspaces ('overwritten' in include/psnd.h); what it returns is the same bits on both.  No allocator involved."""
    results = []
    for byte in patterns:
        bufs = {k: _fill(torch.empty(shp, dtype=dt, device=DEV), byte) for k, (shp, dt) in shapes.items()}
        torch.cuda.synchronize()
        out = call(bufs)
        torch.cuda.synchronize()
        results.append(P.to_cpu([bufs[k] for k in out]))
    bad = P.not_finite(results, patterns) + P.differences(results, patterns)
    assert not bad, 'a caller-owned buffer is read before it is written:\n  ' + '\n  '.join(bad[:20])


def test_grad_pack_unpack_sumsq_at_an_odd_length():
    """psnd_grad_pack_bf16 / _unpack_bf16 (n = 8 x 1237) and psnd_grad_sumsq over tensors of odd lengths (partials in double, coef)"""
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    from pytorch_sound_amd.optim import Adam
    torch.manual_seed(9)
    n = 8 * 1237
    x = torch.randn(n, device=DEV)
    st = stream_ptr(torch.device(DEV))

    def pack(b):
        check(lib().psnd_grad_pack_bf16(ptr(x), ptr(b['packed']), n, 0.125, st), 'pack')
        check(lib().psnd_grad_unpack_bf16(ptr(b['packed']), ptr(b['back']), n, 4.0, st), 'unpack')
        return ['packed', 'back']

    _on_prefilled(pack, {'packed': ((n,), torch.bfloat16), 'back': ((n,), torch.float32)})

    params = [torch.nn.Parameter(torch.randn(s, device=DEV)) for s in ((9973,), (3, 7), (1,), (70001,))]
    for p in params:
        p.grad = torch.randn_like(p)
    opt = Adam(params, lr=1e-3)
    opt.fused_clip = (0.7, 5.0)

    def fn():
        opt.step()
        return [[p.detach() for p in params], [[opt.state[p][k] for k in ('step', 'exp_avg', 'exp_avg_sq')] for p in params]]

    # the optimizer is stateful: three runs from the same start
    start = [p.detach().clone() for p in params]
    results = []

    def fresh():
        with torch.no_grad():
            for p, s in zip(params, start):
                p.copy_(s)
                for k in ('step', 'exp_avg', 'exp_avg_sq'):
                    if p in opt.state:
                        opt.state[p][k].zero_()
        return fn()

    results = P.run_on_patterns(fresh)
    bad = P.not_finite(results) + P.differences(results)
    assert not bad, bad


# ---- caller-owned workspaces through the C ABI -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,C,T,relu,with_res', [(3, 256, 700, False, True), (4, 16, 33, True, False)])
def test_cabi_groupnorm1_workspaces(N, C, T, relu, with_res):
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    torch.manual_seed(N + C)
    x, res, gy = (torch.randn(N, C, T, device=DEV) for _ in range(3))
    res = res if with_res else None
    gamma, beta = 1 + 0.2 * torch.randn(C, device=DEV), 0.1 * torch.randn(C, device=DEV)
    st = stream_ptr(torch.device(DEV))

    def call(b):
        check(lib().psnd_groupnorm1_fwd(ptr(x), ptr(res), ptr(gamma), ptr(beta), N, C, T, 1e-5, int(relu), ptr(b['y']), ptr(b['stats']),
                                        ptr(b['ws']), st), 'psnd_groupnorm1_fwd')
        check(lib().psnd_groupnorm1_bwd(ptr(gy), ptr(x), ptr(res), ptr(gamma), ptr(b['y']), ptr(b['stats']), N, C, T, int(relu), ptr(b['gx']),
                                        ptr(b['gg']), ptr(b['gb']), ptr(b['ws2']), st), 'psnd_groupnorm1_bwd')
        return ['y', 'stats', 'gx', 'gg', 'gb']

    f32, f64 = torch.float32, torch.float64
    _on_prefilled(call, {'y': ((N, C, T), f32), 'stats': ((N, 2), f32), 'ws': ((N, 2 * C), f64), 'ws2': ((N, 2 * C), f64),
                         'gx': ((N, C, T), f32), 'gg': ((C,), f32), 'gb': ((C,), f32)})


def test_cabi_wgrad_slabs():
    """psnd_conv1d_cl_wgrad and psnd_conv1d_cl_wgrad_multi (convs of three shapes in one launch): gw_part / gbias_part, every slab entry"""
    from pytorch_sound_amd import _lib, cl
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    torch.manual_seed(5)
    N, L, HP = 6, 173, 25
    Lp = cl.CLShape(N, L, HP).Lp
    specs = [(256, 256, 3, -1, 1), (256, 256, 3, -5, 5), (520, 256, 3, -1, 1), (64, 128, 7, -9, 3)]
    S = int(lib().psnd_conv1d_cl_wgrad_multi_splits(N, Lp, 256, 256, 3, 3))
    ops = []
    for Ca, Cb, k, off0, dstep in specs:
        g = torch.zeros(N, Lp, Cb, device=DEV, dtype=torch.bfloat16)
        x = torch.zeros(N, Lp, Ca, device=DEV, dtype=torch.bfloat16)
        g[:, HP:HP + L] = torch.randn(N, L, Cb, device=DEV).to(torch.bfloat16)
        x[:, HP:HP + L] = torch.randn(N, L, Ca, device=DEV).to(torch.bfloat16)
        ops.append((g, x))
    st = stream_ptr(torch.device(DEV))
    shapes = {}
    for i, (Ca, Cb, k, off0, dstep) in enumerate(specs):
        S1 = int(lib().psnd_conv1d_cl_wgrad_splits(N, Lp, Ca, Cb, k))
        shapes.update({'gw%d' % i: ((S, k, Cb, Ca), torch.float32), 'gb%d' % i: ((S, Cb), torch.float32),
                       'one_gw%d' % i: ((S1, k, Cb, Ca), torch.float32), 'one_gb%d' % i: ((S1, Cb), torch.float32)})

    def call(b):
        arr = (_lib.WgradDesc * len(specs))()
        for i, (d, (Ca, Cb, k, off0, dstep), (g, x)) in enumerate(zip(arr, specs, ops)):
            d.g, d.xa, d.gw_part, d.gbias_part = g.data_ptr(), x.data_ptr(), b['gw%d' % i].data_ptr(), b['gb%d' % i].data_ptr()
            d.off0, d.dstep, d.Ca, d.Cb, d.k, d.splits = off0, dstep, Ca, Cb, k, S
            check(lib().psnd_conv1d_cl_wgrad(ptr(g), None, None, 1.0, ptr(x), N, Lp, Ca, Cb, k, off0, dstep, ptr(b['one_gw%d' % i]),
                                             ptr(b['one_gb%d' % i]), None, st), 'psnd_conv1d_cl_wgrad')
        check(lib().psnd_conv1d_cl_wgrad_multi(ctypes.addressof(arr), len(specs), N, Lp, st), 'psnd_conv1d_cl_wgrad_multi')
        return sorted(shapes)

    _on_prefilled(call, shapes)


@pytest.mark.parametrize('N,Lp,C,lo,hi', [(3, 40, 32, 5, 33), (16, 306, 256, 25, 281), (2, 8200, 64, 25, 8175), (1, 24, 8, 3, 3)])
def test_cabi_colsum_part(N, Lp, C, lo, hi):
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    torch.manual_seed(N + Lp + C)
    g = torch.randn(N, Lp, C, device=DEV).to(torch.bfloat16)
    rows = N * Lp
    st = stream_ptr(torch.device(DEV))

    def call(b):
        check(lib().psnd_cl_colsum(ptr(g), rows, C, Lp, lo, hi, ptr(b['part']), ptr(b['out']), st), 'colsum')
        check(lib().psnd_cl_colsum(ptr(g), rows, C, 0, 0, 0, ptr(b['part_all']), ptr(b['out_all']), st), 'colsum')
        return ['out', 'out_all']

    n = int(lib().psnd_cl_colsum_splits(rows, C)) * C
    _on_prefilled(call, {'part': ((n,), torch.float32), 'out': ((C,), torch.float32), 'part_all': ((n,), torch.float32), 'out_all': ((C,), torch.float32)})


def test_cabi_loss_block_partials():
    """psnd_l1_loss_fwd (part, out) at n = 16385 and 5; psnd_stft_loss_partial: every entry of part[(n B + b) 3 + i] is written"""
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    torch.manual_seed(8)
    st = stream_ptr(torch.device(DEV))
    for n in (16385, 5, 513 * 173 * 3):
        a, c = torch.randn(n, device=DEV), torch.randn(n, device=DEV)

        def call(b):
            check(lib().psnd_l1_loss_fwd(ptr(a), ptr(c), n, ptr(b['part']), ptr(b['out']), st), 'psnd_l1_loss_fwd')
            return ['part', 'out']

        _on_prefilled(call, {'part': ((int(lib().psnd_l1_loss_blocks(n)),), torch.float64), 'out': ((), torch.float32)})
    for N, KF in ((3, 513 * 21), (2, 1025 * 7), (1, 257 * 3)):
        p, t = torch.rand(N, KF, device=DEV) * 3, torch.rand(N, KF, device=DEV) * 3
        B = int(lib().psnd_stft_loss_blocks(KF))

        def call(b):
            check(lib().psnd_stft_loss_partial(ptr(p), ptr(t), N, KF, 1e-2, ptr(b['part']), st), 'psnd_stft_loss_partial')
            return ['part']

        _on_prefilled(call, {'part': ((N, B, 3), torch.float64)})


@pytest.mark.parametrize('N,H,C,T,masked,bf16', [(2, 4, 256, 173, True, 0), (2, 2, 96, 77, False, 0), (3, 4, 64, 50, True, 1)])
def test_cabi_mha_bwd_workspaces(N, H, C, T, masked, bf16):
    """psnd_mha_fwd (out, att, stats) and psnd_mha_bwd (delta scratch, gkvq), with the attention tensor's gradient"""
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    torch.manual_seed(T)
    kvq, gout = 0.5 * torch.randn(N, 3 * C, T, device=DEV), torch.randn(N, C, T, device=DEV)
    gatt = 0.1 * torch.randn(H * N, T, T, device=DEV)
    mask = None
    if masked:
        lens = torch.linspace(T, max(T // 3, 8), N).long()
        mask = (torch.arange(T)[None, :] >= lens[:, None]).to(torch.uint8).to(DEV).contiguous()
    st = stream_ptr(torch.device(DEV))

    def call(b):
        check(lib().psnd_mha_fwd(ptr(kvq), ptr(mask), N, H, C, T, ptr(b['out']), ptr(b['att']), ptr(b['stats']), bf16, st), 'psnd_mha_fwd')
        check(lib().psnd_mha_bwd(ptr(kvq), ptr(mask), ptr(b['out']), ptr(b['att']), ptr(b['stats']), ptr(gout), ptr(gatt), N, H, C, T,
                                 ptr(b['delta']), ptr(b['gkvq']), bf16, st), 'psnd_mha_bwd')
        return ['out', 'att', 'gkvq']

    f32 = torch.float32
    _on_prefilled(call, {'out': ((N, C, T), f32), 'att': ((H * N, T, T), f32), 'stats': ((H * N, T, 2), f32), 'delta': ((H * N, T), f32),
                         'gkvq': ((N, 3 * C, T), f32)})
