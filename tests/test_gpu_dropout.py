"""Dropout on HIP tensors: formed inside the GroupNorm kernels (psnd_groupnorm1_drop_*), never by a library kernel.

The mask is a fixed function, recomputed here in numpy: element i of the contiguous (N, C, T) tensor is kept iff word i % 4 of
Philox4x32-10(counter = (q lo, q hi, call lo, call hi) with q = i // 4, key = (seed lo, seed hi)) is >= thr = min(2^32 - 1,
floor(p * 2^32)); kept elements are scaled by 1 / (1 - p), formed in fp32.  {seed, call} live in device memory
(kernels.dropout_seed / dropout_state), every application takes the pair and counts the call (psnd_rng_next).

Tolerances: those tests/test_gpu_modules.py applies to the same kernels without dropout - GroupNorm1 alone 3e-6 of max (output) and
2e-5 of max (gradients) against float64; the attention + feed-forward block 3e-5 of max (output) and 2e-4 of max (gradients)."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

M32 = 0xffffffff


# ---- the test's own Philox4x32-10 ------------------------------------------------------------------------------------------------
def philox4x32_10(ctr, key):
    """ctr: (n, 4) array of 32-bit words, key: two 32-bit words -> (n, 4) uint32"""
    c = [np.asarray(ctr)[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]) & M32, int(key[1]) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]          # 32 x 32 -> 64 bits: no overflow
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & np.uint64(M32), p1 >> np.uint64(32), p1 & np.uint64(M32)
        c = [h1 ^ c[1] ^ np.uint64(k0), l1, h0 ^ c[3] ^ np.uint64(k1), l0]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c, 1).astype(np.uint32)


def drop_thr(p):
    return min(2 ** 32 - 1, int(np.floor(np.float64(p) * 2.0 ** 32)))


def drop_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(shape, seed, call, p):
    """bool array of `shape`: the elements dropout application (seed, call) of rate p keeps"""
    n = int(np.prod(shape))
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q & np.uint64(M32), q >> np.uint64(32), np.full_like(q, call & M32), np.full_like(q, (call >> 32) & M32)], 1)
    words = philox4x32_10(ctr, (seed & M32, (seed >> 32) & M32)).reshape(-1)[:n]
    return (words >= np.uint32(drop_thr(p))).reshape(shape)


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((M32, M32, M32, M32), (M32, M32), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_numpy_philox_known_answers():
    """the published known-answer vectors of Philox4x32-10 (needs no GPU)"""
    for ctr, key, out in KAT:
        assert tuple(int(w) for w in philox4x32_10(np.array([ctr], dtype=np.uint64), key)[0]) == out
    got = philox4x32_10(np.array([k[0] for k in KAT[:1] * 3], dtype=np.uint64), KAT[0][1])      # rows are independent
    assert all(tuple(int(w) for w in r) == KAT[0][2] for r in got)
    assert drop_thr(0.5) == 1 << 31 and drop_thr(0.1) == 429496729 and drop_thr(1.0 - 2.0 ** -40) == M32


# ---- helpers -------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _global_generators_untouched():
    """these tests seed torch (and the Trainer numpy) to build their modules: the process-wide generators are handed back as they were found,
    so tests that run later and draw from them unseeded see the numbers they would see without this file"""
    cpu, host = torch.get_rng_state(), np.random.get_state()
    gpu = torch.cuda.get_rng_state(_dev()) if torch.cuda.is_available() else None
    yield
    torch.set_rng_state(cpu)
    np.random.set_state(host)
    if gpu is not None:
        torch.cuda.set_rng_state(gpu, _dev())


def _mixed_seed(shape, p, call=0):
    """the first seed whose mask holds kept AND dropped elements in every sample: GroupNorm of an all-kept sample of ones is 0 everywhere"""
    for seed in range(1000, 1100):
        k = keep_mask(shape, seed, call, p).reshape(shape[0], -1)
        if np.all(k.any(1) & ~k.all(1)):
            return seed
    raise AssertionError('no usable seed')


def _mask_of_ones(shape, p, misaligned=False):
    """y > 0 of GroupNorm1(ones * keep * scale + zeros): the mask the kernels drew"""
    from pytorch_sound_amd import kernels as K
    dev, n = _dev(), int(np.prod(shape))
    if misaligned:                                     # a contiguous view that starts 4 bytes into its storage: no 16-byte rows
        x = torch.ones(n + 1, device=dev)[1:].view(shape)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    else:
        x = torch.ones(shape, device=dev)
    C = shape[1]
    y = K.GroupNorm1.apply(x, torch.zeros(shape, device=dev), torch.ones(C, device=dev), torch.zeros(C, device=dev), 1e-5, False, None, p)
    return (y > 0).cpu().numpy()


# ---- 1. the mask is the specified function -----------------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('shape,misaligned', [((1, 4, 4), False), ((3, 8, 50), False), ((2, 16, 64), False), ((2, 256, 173), False),
                                              ((2, 16, 64), True)])
def test_mask_is_the_specified_function(shape, misaligned, p):
    from pytorch_sound_amd import kernels as K
    K.dropout_seed(_mixed_seed(shape, p, call=7), call=7)
    seed, call = K.dropout_state()
    assert call == 7
    got = _mask_of_ones(shape, p, misaligned)
    want = keep_mask(shape, seed, call, p)
    assert np.array_equal(got, want), '%d of %d elements differ' % (int((got != want).sum()), got.size)
    assert K.dropout_state() == (seed, call + 1)
    if shape == (2, 256, 173):
        n = got.size
        frac = got.sum() / n
        print('p=%.1f: kept %.5f of %d (bound %.5f)' % (p, frac, n, 5 * np.sqrt(p * (1 - p) / n)))
        assert abs(frac - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)


def test_mask_counter_beyond_32_bits():
    """seed and call use all 64 bits of their words (the Trainer puts the rank into bits 48.. of call)"""
    from pytorch_sound_amd import kernels as K
    seed, call, shape = 0xfedcba9876543210, (3 << 48) + (5 << 20) + 9, (3, 8, 50)
    K.dropout_seed(seed, call=call)
    assert K.dropout_state() == (seed, call)
    assert np.array_equal(_mask_of_ones(shape, 0.5), keep_mask(shape, seed, call, 0.5))


# ---- 2. values and gradients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('N,C,T', [(3, 8, 50), (2, 256, 173)])
def test_groupnorm1_drop_vs_float64(N, C, T, relu):
    from pytorch_sound_amd import kernels as K
    dev, p = _dev(), 0.1
    rs = np.random.RandomState(N * C + T)
    x0, r0, g0 = (rs.randn(N, C, T).astype(np.float32) for _ in range(3))
    x0 = x0 * 2 + 0.7
    gamma0, beta0 = (rs.randn(C) * 0.3 + 1).astype(np.float32), (rs.randn(C) * 0.2).astype(np.float32)
    K.dropout_seed(11 + T, call=3)
    seed, call = K.dropout_state()
    keep = keep_mask((N, C, T), seed, call, p)

    x, r, gamma, beta = (torch.from_numpy(a).to(dev).requires_grad_(True) for a in (x0, r0, gamma0, beta0))
    y = K.GroupNorm1.apply(x, r, gamma, beta, 1e-5, relu, None, p)
    (y * torch.from_numpy(g0).to(dev)).sum().backward()
    torch.cuda.synchronize()

    xr, rr, gr, br = (torch.from_numpy(a).double().requires_grad_(True) for a in (x0, r0, gamma0, beta0))
    m = torch.from_numpy(keep).double() * drop_scale(p)
    yr = torch.nn.functional.group_norm(xr * m + rr, 1, gr, br, 1e-5)
    if relu:
        yr = torch.relu(yr)
    (yr * torch.from_numpy(g0).double()).sum().backward()

    def err(a, b):
        return float((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max())
    errs = dict(y=err(y, yr), gx=err(x.grad, xr.grad), gres=err(r.grad, rr.grad), ggamma=err(gamma.grad, gr.grad), gbeta=err(beta.grad, br.grad))
    print((N, C, T), 'relu' if relu else '', ' '.join('%s %.1e' % kv for kv in errs.items()))
    assert errs['y'] <= 3e-6
    for k in ('gx', 'gres', 'ggamma', 'gbeta'):
        assert errs[k] <= 2e-5, (k, errs[k])
    dropped = torch.from_numpy(~keep)
    assert bool((x.grad.cpu()[dropped] == 0).all()), 'gx is an exact zero where the element was dropped'
    assert float((r.grad.cpu()[dropped] != 0).float().mean()) > 0.99, 'the residual\'s gradient is not masked'
    assert x.grad.data_ptr() != r.grad.data_ptr()


# ---- 3. module level --------------------------------------------------------------------------------------------------------------------
class _FixedMask(torch.nn.Module):
    """stands in for nn.Dropout in the float64 yardstick: the numpy mask times the fp32 scale"""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return x * self.m


FORBIDDEN = ('native_dropout', 'native_dropout_backward', 'dropout', 'bernoulli', 'bernoulli_', 'rand_like')


def _no_library_dropout():
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_flatten
    packets = {getattr(torch.ops.aten, n) for n in FORBIDDEN}

    class Guard(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func.overloadpacket in packets and any(isinstance(a, torch.Tensor) and a.is_cuda for a in tree_flatten((args, kwargs))[0]):
                raise AssertionError('%s reached with a HIP tensor' % func)
            return func(*args, **(kwargs or {}))
    return Guard()


def _block(p, seed=0):
    from pytorch_sound_amd.models.modules import MultiHeadAttention, PointwiseFeedForward
    torch.manual_seed(seed)
    mha, ffn = MultiHeadAttention(64, 4, p), PointwiseFeedForward(64, p)
    with torch.no_grad():
        for m in (mha, ffn):
            m.layernorm.weight.copy_(1 + 0.2 * torch.randn(64))
            m.layernorm.bias.copy_(0.1 * torch.randn(64))
    return mha, ffn


def _block_data(N=3, T=50):
    rs = np.random.RandomState(5)
    lens = np.array([50, 30, 17])
    mask = torch.from_numpy(np.arange(T)[None, :] >= lens[:, None])
    x0 = torch.from_numpy((0.5 * rs.randn(N, 64, T)).astype(np.float32)) * (~mask).unsqueeze(1)
    gy = torch.from_numpy(rs.randn(N, 64, T).astype(np.float32))
    return x0, mask, gy


def _run_block(mha, ffn, x0, mask, gy):
    for m in (mha, ffn):
        for q in m.parameters():
            q.grad = None
    x = x0.detach().clone().requires_grad_(True)
    h, _ = mha(x, mask)
    y = ffn(h)
    (y * gy).sum().backward()
    grads = {('mha.' + k): q.grad for k, q in mha.named_parameters()}
    grads.update({('ffn.' + k): q.grad for k, q in ffn.named_parameters()})
    return y.detach(), x.grad, grads


def test_block_with_dropout_vs_float64_and_no_library_dropout():
    from pytorch_sound_amd import kernels as K
    dev, p = _dev(), 0.1
    mha, ffn = _block(p)
    ref = tuple(copy.deepcopy(m).double() for m in (mha, ffn))
    mha, ffn = mha.to(dev).train(), ffn.to(dev).train()
    x0, mask, gy = _block_data()
    K.dropout_seed(2024, call=40)
    seed, c0 = K.dropout_state()
    with _no_library_dropout():
        y, gx, gp = _run_block(mha, ffn, x0.to(dev), mask.to(dev), gy.to(dev))
        torch.cuda.synchronize()
    assert K.dropout_state() == (seed, c0 + 2)

    for m, c in zip(ref, (c0, c0 + 1)):
        m.train()
        m.drop_out = _FixedMask(torch.from_numpy(keep_mask(tuple(x0.shape), seed, c, p)).double() * drop_scale(p))
    yr, gxr, gpr = _run_block(ref[0], ref[1], x0.double(), mask, gy.double())

    def err(a, b):
        return float((a.cpu().double() - b).abs().max() / b.abs().max())
    worst = max(gp, key=lambda k: err(gp[k], gpr[k]))
    print('y %.1e  gx %.1e  worst parameter gradient %s %.1e' % (err(y, yr), err(gx, gxr), worst, err(gp[worst], gpr[worst])))
    assert err(y, yr) <= 3e-5
    assert err(gx, gxr) <= 2e-4
    for k in gp:
        assert err(gp[k], gpr[k]) <= 2e-4, (k, err(gp[k], gpr[k]))


# ---- 4. seeding ---------------------------------------------------------------------------------------------------------------------------
def test_seeding():
    from pytorch_sound_amd import kernels as K
    shape, p = (3, 8, 50), 0.5
    K.dropout_seed(123)
    a0, a1 = _mask_of_ones(shape, p), _mask_of_ones(shape, p)
    K.dropout_seed(123)
    b0 = _mask_of_ones(shape, p)
    K.dropout_seed(124)
    c0 = _mask_of_ones(shape, p)
    assert np.array_equal(a0, b0), 'the same seed gives the same bits'
    assert not np.array_equal(a0, a1), 'two consecutive applications draw different masks'
    assert not np.array_equal(a0, c0), 'different seeds give different masks'
    K.dropout_seed(123, call=1)
    assert np.array_equal(_mask_of_ones(shape, p), a1)


# ---- 5. eval mode --------------------------------------------------------------------------------------------------------------------------
def test_eval_mode_is_the_rate_zero_module_and_draws_nothing():
    from pytorch_sound_amd import kernels as K
    dev = _dev()
    drop, plain = _block(0.1), _block(0.0)
    assert drop[0].drop_out is not None and plain[0].drop_out is None
    for a, b in zip(drop, plain):
        b.load_state_dict(a.state_dict())
        a.to(dev).eval(), b.to(dev).eval()
    x0, mask, gy = _block_data()
    K.dropout_seed(9, call=100)
    with _no_library_dropout():
        y, gx, gp = _run_block(drop[0], drop[1], x0.to(dev), mask.to(dev), gy.to(dev))
    y0, gx0, gp0 = _run_block(plain[0], plain[1], x0.to(dev), mask.to(dev), gy.to(dev))
    assert torch.equal(y, y0) and torch.equal(gx, gx0)
    for k in gp:
        assert torch.equal(gp[k], gp0[k]), k
    assert K.dropout_state() == (9, 100)


# ---- 6. graph replay ---------------------------------------------------------------------------------------------------------------------
def test_graph_replay_draws_fresh_masks():
    from pytorch_sound_amd import kernels as K
    dev, p = _dev(), 0.1
    mha, ffn = _block(p)
    mha, ffn = mha.to(dev).train(), ffn.to(dev).train()
    x0, mask, gy = (t.to(dev) for t in _block_data())
    K.dropout_seed(1)                                      # the state exists before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            _run_block(mha, ffn, x0, mask, gy)
    torch.cuda.current_stream().wait_stream(side)
    for m in (mha, ffn):
        for q in m.parameters():
            q.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _run_block(mha, ffn, x0, mask, gy)

    def snapshot(o):
        return [o[0].clone(), o[1].clone()] + [o[2][k].clone() for k in sorted(o[2])]

    s = 77
    K.dropout_seed(s)
    replays = []
    for i in range(3):
        graph.replay()
        replays.append(snapshot(out))
        assert K.dropout_state() == (s, 2 * (i + 1))
    for i in range(3):
        K.dropout_seed(s, call=2 * i)
        eager = snapshot(_run_block(mha, ffn, x0, mask, gy))
        assert all(torch.equal(a, b) for a, b in zip(replays[i], eager)), 'replay %d is not the eager step at call %d' % (i, 2 * i)
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[1][0], replays[2][0])
    assert not torch.equal(replays[0][0], replays[2][0])


# ---- 7. first use inside a capture --------------------------------------------------------------------------------------------------
def test_first_use_inside_a_capture_raises():
    from pytorch_sound_amd import kernels as K
    dev = _dev()
    x, r = torch.ones(1, 4, 4, device=dev), torch.zeros(1, 4, 4, device=dev)
    g, b = torch.ones(4, device=dev), torch.zeros(4, device=dev)
    torch.cuda.synchronize()
    K._dropout_reset()                                     # as in a process that never applied or seeded dropout
    try:
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(K.PsndError, match='dropout_seed'):
            with torch.cuda.graph(graph):
                r = r + 1                                  # (the capture holds something: an empty graph is a special case of its own)
                K.GroupNorm1.apply(x, r, g, b, 1e-5, False, None, 0.1)
        assert dev.index not in K._DROPOUT_STATE, 'no state was created inside the capture'
    finally:
        K.dropout_seed(torch.initial_seed())
    assert K.dropout_state() == (torch.initial_seed() & ((1 << 64) - 1), 0), 'nothing was launched: the call counter stands at 0'


def test_first_use_without_seeding_takes_torch_initial_seed():
    from pytorch_sound_amd import kernels as K
    torch.cuda.synchronize()
    K._dropout_reset()
    before = torch.get_rng_state()
    got = _mask_of_ones((3, 8, 50), 0.5)
    assert torch.equal(before, torch.get_rng_state()), 'the host generator was not consumed'
    assert np.array_equal(got, keep_mask((3, 8, 50), torch.initial_seed(), 0, 0.5))
    assert K.dropout_state() == (torch.initial_seed() & ((1 << 64) - 1), 1)


# ---- the Trainer seeds the state -----------------------------------------------------------------------------------------------------
def test_trainer_seeds_the_dropout_state(tmp_path):
    """seed from the Trainer's seed, call from rank and step: ranks draw different masks, a resumed run does not repeat step 0's"""
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd.trainer import Trainer
    model = torch.nn.Conv1d(2, 2, 1).to(_dev())
    K.dropout_seed(99, call=99)
    tr = Trainer(model, torch.optim.SGD(model.parameters(), lr=0.1), [], [], max_step=1, valid_max_step=1, save_interval=1, log_interval=1,
                 save_dir=str(tmp_path), seed=5)
    assert (tr.seed, tr.step) == (5, 0)
    assert K.dropout_state() == (5, 0)
