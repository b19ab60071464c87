"""InversePreEmphasis and VolNormConv on HIP tensors (psnd_ipreemph_*, psnd_volnorm_*): every call runs under a guard that raises when
a HIP tensor reaches the ops the old paths used (MIOpen's RNN; torch.std / torch.cat per hop).

Tolerances.  InversePreEmphasis forward: the distance of the CPU fp32 nn.RNN from the float64 recurrence on the same fp32 input is
computed in the test; the GPU result may be four times as far (a different tanh is amplified by the same 1 / (1 - |w_hh|)).  Backward: four
times the CPU fp32 autograd's own distance (relative to the maximum) from float64 autograd.  Golden values: the existing CPU tests' numbers
(atol 1e-6; rtol 1e-6 / atol 1e-7 for VolNormConv)."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from pytorch_sound_amd import kernels as K
from pytorch_sound_amd.models.sound import InversePreEmphasis, VolNormConv, ipreemph_warm, volnorm_layout

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORBIDDEN = ('aten.rnn_tanh', 'aten._rnn', 'aten.miopen_rnn', 'aten._cudnn_rnn', 'aten.std', 'aten.var', 'aten.cat')
SPAN = K.IPREEMPH_SPAN
# one seam between workgroup spans, three 32-sample chunks (seams between lanes) and a ragged tail of 17; T shorter than the warm-up (608 at
# 0.97); T = 1.  A few thousand samples: the CPU autograd references walk every step in python-visible nodes
SHAPES_T = (SPAN + 3 * 32 + 17, 300, 1)


class _Guard(TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = str(func)
        if name.startswith(FORBIDDEN):
            flat = torch.utils._pytree.tree_leaves((args, kwargs or {}))
            if any(isinstance(a, torch.Tensor) and a.is_cuda for a in flat):
                raise AssertionError('%s reached with a HIP tensor' % name)
        return func(*args, **(kwargs or {}))


def _module(w_hh, coef=0.97, w_ih=1.0):
    m = InversePreEmphasis(coef)
    m.rnn.weight_ih_l0.data.fill_(w_ih)
    m.rnn.weight_hh_l0.data.fill_(w_hh)
    return m


def _inputs(T, seed=0):
    """(9, 1, T): three clips each of amplitude 0.01 (slow decay: the seams' worst case), amplitude 1, zeros followed by one impulse"""
    g = torch.Generator().manual_seed(seed + T)
    x = torch.randn(9, 1, T, generator=g)
    x[:3] *= 0.01
    x[6:] = 0
    x[6:, 0, T // 3] = 1.0
    return x


def _scan64(x, w_ih, w_hh):
    """the recurrence in float64 from the fp32 input and the fp32 weights"""
    xs = x[:, 0].double().numpy() * float(np.float32(w_ih))
    c = float(np.float32(w_hh))
    y = np.empty_like(xs)
    h = np.zeros(xs.shape[0])
    for t in range(xs.shape[1]):
        h = np.tanh(xs[:, t] + c * h)
        y[:, t] = h
    return torch.from_numpy(y)[:, None]


@pytest.fixture(scope='module')
def golden_sound(golden):
    return golden('sound')


def test_inverse_preemphasis_golden(golden_sound):
    g = golden_sound
    ipe = InversePreEmphasis(0.97).to(DEV)
    x = torch.from_numpy(g['preemph/y'])[:, :, :256].to(DEV)
    with _Guard(), torch.no_grad():
        y = ipe(x)
    assert y.shape == g['ipreemph/y'].shape and y.dtype == torch.float32
    assert np.allclose(y.cpu().numpy(), g['ipreemph/y'], atol=1e-6)
    with _Guard():                                                           # grad mode: the parameters require a gradient
        y2 = ipe(x)
    assert y2.requires_grad and torch.equal(y2.detach(), y)
    assert set(ipe.state_dict()) == {'rnn.weight_ih_l0', 'rnn.weight_hh_l0'}
    with pytest.raises(RuntimeError):
        ipe(torch.zeros(2, 2, 64, device=DEV))
    with pytest.raises(RuntimeError):
        ipe(torch.zeros(2, 1, 64, device=DEV, dtype=torch.int32))
    with pytest.raises(RuntimeError):
        InversePreEmphasis(0.97)(x)                                          # parameters on the CPU, input on the GPU


@pytest.mark.parametrize('w_hh', [0.97, 0.5, -0.97, 1.0, 1.5])
def test_inverse_preemphasis_against_float64(w_hh):
    """Measured on an MI355X, max |y - float64| over the shapes, CPU fp32 nn.RNN / GPU: amplitude 0.01: 2.1e-8 / 3.7e-9 at +-0.97, 6.7e-8 / 7.4e-9 at 1,
    1.4e-7 / 3.0e-8 at 1.5; amplitude 1: 6.4e-8 ... 1.0e-7 / 3.0e-8 below 1, 1.2e-6 / 3.0e-8 at 1.5; impulse: 2.1e-8 ... 5.2e-8 / 2.0e-8 ... 2.9e-8.
    T = 1: equal (both are the rounded tanh).  The GPU figure is the rounding of the fp32 output: the recurrence itself runs in fp64."""
    assert (ipreemph_warm(w_hh) == K.IPREEMPH_SEQ) == (abs(w_hh) >= 1)
    cpu, gpu = _module(w_hh), _module(w_hh).to(DEV)
    for T in SHAPES_T:
        x = _inputs(T)
        ref = _scan64(x, 1.0, w_hh)
        with torch.no_grad():
            y_cpu = cpu(x)
            with _Guard():
                y = gpu(x.to(DEV)).cpu()
        for name, sl in (('amplitude 0.01', slice(0, 3)), ('amplitude 1', slice(3, 6)), ('impulse', slice(6, 9))):
            d_cpu = (y_cpu[sl].double() - ref[sl]).abs().max().item()
            d_gpu = (y[sl].double() - ref[sl]).abs().max().item()
            print('w_hh=%g T=%d %s: cpu fp32 %.3e gpu %.3e' % (w_hh, T, name, d_cpu, d_gpu))
            assert d_gpu <= 4 * d_cpu, 'w_hh=%g T=%d %s: GPU %.3e from float64, CPU fp32 nn.RNN %.3e' % (w_hh, T, name, d_gpu, d_cpu)


def test_inverse_preemphasis_instances_agree_at_the_seams():
    """the time-parallel instance (warm-up from h = 0) against the sequential one on the same input: 2 |w_hh|^W <= 2^-25 plus the output's
    fp32 rounding (|y| <= 1: 2^-24), at every sample - the seams included"""
    gpu = _module(0.97).to(DEV)
    x = _inputs(3 * SPAN + 17).to(DEV)
    w_ih, w_hh = gpu.rnn.weight_ih_l0.detach(), gpu.rnn.weight_hh_l0.detach()
    with _Guard():
        y_auto = gpu(x).detach()
        y_par = K.InversePreEmphasisFn.apply(x, w_ih, w_hh, ipreemph_warm(0.97))
        y_seq = K.InversePreEmphasisFn.apply(x, w_ih, w_hh, K.IPREEMPH_SEQ)
    assert torch.equal(y_auto, y_par)                                        # the kernel's own rule is the host's
    assert (y_par - y_seq).abs().max().item() <= 2.0 ** -25 + 2.0 ** -24


def test_inverse_preemphasis_reads_the_parameters():
    gpu = InversePreEmphasis(0.97).to(DEV)
    x = _inputs(2000)
    for c in (0.5, 0.9, 1.0):                                                # .data.fill_ moves no version counter; 1.0: the other instance
        gpu.rnn.weight_hh_l0.data.fill_(c)
        with _Guard(), torch.no_grad():
            y = gpu(x.to(DEV)).cpu()
        assert (y.double() - _scan64(x, 1.0, c)).abs().max().item() < 1e-6, c
    sd = {'rnn.weight_ih_l0': torch.full((1, 1), 0.8), 'rnn.weight_hh_l0': torch.full((1, 1), -0.6)}
    gpu.load_state_dict(sd)
    with _Guard(), torch.no_grad():
        y = gpu(x.to(DEV)).cpu()
    assert (y.double() - _scan64(x, 0.8, -0.6)).abs().max().item() < 1e-6


def _rel_distance(v, ref):
    """max |v - ref| / max |ref| over the entries of the float64 reference that fp32 can hold.  With |w_hh| > 1 the gradient grows by w_hh per
    step through silence (y = 0: the lead-in of the impulse clips) and leaves first the fp32 and then the float64 range: where the
    reference is beyond fp32 or not finite, `v` must not be a finite number either (inf if it is not in that case); a NaN among the
    compared entries is an infinite distance."""
    v, ref = v.double().reshape(-1), ref.reshape(-1)
    beyond = ~torch.isfinite(ref) | (ref.abs() > 1e39)
    if bool((beyond & torch.isfinite(v)).any()):
        return float('inf')
    held = torch.isfinite(ref) & (ref.abs() < 1e38)
    if not bool(held.any()):
        return 0.0
    d = (v[held] - ref[held]).abs().max().item() / (ref[held].abs().max().item() or 1.0)      # T = 1: the gradient of w_hh is exactly 0
    return d if d == d else float('inf')


def _backward(module, x, gy):
    x = x.clone().requires_grad_(True)
    module.zero_grad()
    (module(x) * gy).sum().backward()
    return x.grad, module.rnn.weight_ih_l0.grad.clone(), module.rnn.weight_hh_l0.grad.clone()


@pytest.mark.parametrize('w_hh', [0.97, 0.5, -0.97, 1.0, 1.5])
def test_inverse_preemphasis_backward(w_hh):
    """gx, g_w_ih, g_w_hh against CPU float64 autograd of nn.RNN(...).double(); allowance: four times the CPU fp32 autograd's distance.
    Measured on an MI355X at T = 8305, relative to the maximum, CPU fp32 autograd / GPU: gx 5e-8 ... 2e-5 / 3e-8 ... 8e-8; g_w_ih 1.8e-6 ... 1.3e-5 /
    1.4e-8 ... 6.8e-7; g_w_hh 3e-7 ... 1.2e-5 / 5e-9 ... 3e-8 (T = 300: up to 7.0e-6 / 1.5e-6 for g_w_ih at 1).  At 1.5 both weight gradients are
    not finite in float64 either (the impulse clips' silent lead-in, see _rel_distance)."""
    cpu, gpu = _module(w_hh), _module(w_hh).to(DEV)
    cpu64 = _module(w_hh).double()                                           # the fp32 weights, widened
    for T in SHAPES_T:
        x = _inputs(T, seed=1)
        gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(T))
        ref = _backward(cpu64, x.double(), gy.double())
        got_cpu = _backward(cpu, x, gy)
        with _Guard():
            got = _backward(gpu, x.to(DEV), gy.to(DEV))
            again = _backward(gpu, x.to(DEV), gy.to(DEV))
        for a, b in zip(got, again):                                         # bit-equal from run to run (NaN patterns included)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert got[1].shape == (1, 1) and got[2].shape == (1, 1)
        groups = [('gx, ' + n, ref[0][sl], got_cpu[0][sl], got[0][sl]) for n, sl in
                  (('amplitude 0.01', slice(0, 3)), ('amplitude 1', slice(3, 6)), ('impulse', slice(6, 9)))]
        groups += [('g_w_ih', ref[1], got_cpu[1], got[1]), ('g_w_hh', ref[2], got_cpu[2], got[2])]
        for name, r, c, g in groups:
            d_cpu, d_gpu = _rel_distance(c, r), _rel_distance(g.cpu(), r)
            print('w_hh=%g T=%d %s: cpu fp32 %.3e gpu %.3e' % (w_hh, T, name, d_cpu, d_gpu))
            assert d_gpu <= 4 * d_cpu, 'w_hh=%g T=%d %s: GPU %.3e of max from float64, CPU fp32 autograd %.3e' % (w_hh, T, name, d_gpu, d_cpu)


def test_inverse_preemphasis_bf16_and_frozen_weights():
    gpu = _module(0.97).to(DEV)
    x = _inputs(SPAN + 5).to(DEV).bfloat16()
    gy = torch.randn(x.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(3)).bfloat16().float()
    with _Guard():
        g16 = _backward(gpu, x, gy.bfloat16())
        y16 = gpu(x)
        g32 = _backward(gpu, x.float(), gy.bfloat16().float())
        y32 = gpu(x.float())
    assert y16.dtype == torch.bfloat16 and g16[0].dtype == torch.bfloat16
    assert torch.equal(y16, y32.bfloat16()) and torch.equal(g16[0], g32[0].bfloat16())       # one bf16 rounding of the fp32 call
    assert torch.equal(g16[1], g32[1]) and torch.equal(g16[2], g32[2])
    gpu.requires_grad_(False)                                               # only the input's gradient is asked for
    gpu.zero_grad()
    xg = x.float().requires_grad_(True)
    with _Guard():
        (gpu(xg) * gy).sum().backward()
    assert torch.equal(xg.grad, g32[0]) and gpu.rnn.weight_hh_l0.grad is None


def _close(a, b):
    return np.allclose(a, b, rtol=1e-6, atol=1e-7)


def test_volnorm_golden(golden_sound):
    g = golden_sound
    vn = VolNormConv(400, 160, -11.5)
    w = torch.from_numpy(g['volnorm/wav']).to(DEV)
    with _Guard():
        nw = vn.forward(w)
    assert nw.is_cuda and nw.shape == g['volnorm/norm'].shape and _close(nw.cpu().numpy(), g['volnorm/norm'])
    sb = vn.std_buffer
    assert sb.device.type == 'cpu' and sb.dtype == torch.float32 and sb.shape == (23,)
    assert np.allclose(sb.numpy(), g['volnorm/std'], rtol=1e-6)
    with _Guard():
        rv = vn.reverse(nw)
    assert rv.shape == g['volnorm/reverse'].shape and _close(rv.cpu().numpy(), g['volnorm/reverse'])
    assert not nw.requires_grad and not rv.requires_grad


@pytest.mark.parametrize('window,hop', [(400, 160), (400, 219), (400, 200), (100, 300), (1000, 1500)])
def test_volnorm_against_the_cpu_class(window, hop):
    """(400, 219): the last hop starts at L - window - 1 and runs to the end; (400, 200): (L - window) % hop == 0, the last std_buffer entry
    stays 0; (100, 300) and (1000, 1500): hop > window, the last slice clamped at the end / the tail dropped"""
    L = 5000
    if (window, hop) == (400, 219):
        assert (volnorm_layout(L, window, hop)[0] - 1) * hop == L - window - 1
    wav = torch.randn(2, 3, L, generator=torch.Generator().manual_seed(hop)) * torch.linspace(0.05, 1.0, L)
    ref, vn = VolNormConv(window, hop, -11.5), VolNormConv(window, hop, -11.5)
    want = ref.forward(wav)
    with _Guard():
        got = vn.forward(wav.to(DEV).requires_grad_(True))
    assert got.shape == want.shape and not got.requires_grad and _close(got.cpu().numpy(), want.numpy())
    assert vn.std_buffer.shape == ref.std_buffer.shape and vn.std_buffer.device.type == 'cpu'
    assert np.allclose(vn.std_buffer.numpy(), ref.std_buffer.numpy(), rtol=1e-6)
    if (L - window) % hop == 0:
        assert vn.std_buffer[-1] == 0 and vn.std_buffer[-2] > 0
    ref.std_buffer[0] = vn.std_buffer[0] = 2.5                               # reverse reads the buffer, edited or not
    for n in (want.size(-1), window + 2 * hop + 3):                          # and a shorter signal than forward saw
        if n > want.size(-1):
            continue
        with _Guard():
            back = vn.reverse(got[..., :n])
        want_back = ref.reverse(want[..., :n])
        assert back.shape == want_back.shape and _close(back.cpu().numpy(), want_back.numpy())
    with pytest.raises(AssertionError):
        vn.reverse(torch.zeros(1, L + 1, device=DEV))
    h16 = VolNormConv(window, hop, -11.5)
    with _Guard():
        o16 = h16.forward(wav.to(DEV).half())
    assert o16.dtype == torch.float16 and torch.equal(o16, vn.forward(wav.half().float().to(DEV)).half())


def test_volnorm_without_a_hop_raises_as_on_the_cpu():
    for L in (400, 17):
        errs = []
        for dev in ('cpu', DEV):
            vn = VolNormConv(400, 160, -11.5)
            with pytest.raises(Exception) as e:
                vn.forward(torch.zeros(1, L, device=dev))
            errs.append(e.type)
            vn.init_buffer(5000)
            with pytest.raises(Exception) as e:
                vn.reverse(torch.zeros(1, L, device=dev))
            errs.append(e.type)
        assert errs[:2] == errs[2:]


def test_inverse_preemphasis_in_a_captured_graph_follows_the_weights():
    """nothing is read to the host, so the call can be captured; a replay sees the parameters as they are then - across the two instances too"""
    gpu = InversePreEmphasis(0.97).to(DEV)
    x = _inputs(2000)
    static_x = x.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        gpu(static_x)                                                        # library load and allocator warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        static_y = gpu(static_x)
    for c in (0.97, 0.5, 1.0):
        gpu.rnn.weight_hh_l0.data.fill_(c)
        graph.replay()
        assert (static_y.cpu().double() - _scan64(x, 1.0, c)).abs().max().item() < 1e-6, c
