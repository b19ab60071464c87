"""The device-side data-parallel step (hipGraph replay, flat-bucket gradient reduction with the NaN flag riding along, division by
the world size inside the optimizer kernel, collective NaN skip) with TWO ranks sharing the one GPU of the test box over gloo
(PSND_DIST_SHARE_GPU=1; RCCL refuses two ranks on one device): ranks end bit-identical and equal to one process on the full batches."""
import os
import socket
import sys
import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _net():
    torch.manual_seed(7)
    return torch.nn.Sequential(torch.nn.Conv1d(4, 8, 3, padding=1), torch.nn.Tanh(), torch.nn.Conv1d(8, 2, 1))


def _batches(n):
    g = torch.Generator().manual_seed(11)
    return [(torch.randn(4, 4, 16, generator=g), torch.randn(4, 2, 16, generator=g)) for _ in range(n)]


NAN_STEP, STEPS = 5, 9


def _worker(rank, world, port, tmp, q, graph, hip_adam, ddp_mode=None, share=True, clip=False):
    try:
        if ddp_mode is None:
            os.environ.pop('PSND_DDP_GRAPH', None)
        else:
            os.environ['PSND_DDP_GRAPH'] = ddp_mode
        _run(rank, world, port, tmp, q, graph, hip_adam, share, clip)
    except Exception as e:                                                # the parent must not wait for its timeout
        q.put((rank, repr(e)))
        raise


def _run(rank, world, port, tmp, q, graph, hip_adam, share=True, clip=False):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK=str(rank),
                      PSND_DIST_SHARE_GPU='1' if share else '0')
    import torch.distributed as dist
    from pytorch_sound_amd import distributed as pdist, optim as poptim
    from pytorch_sound_amd.trainer import Trainer, LogType
    assert pdist.init_from_env('nccl')                                    # share mode switches to gloo itself
    dev = torch.device('cuda', torch.cuda.current_device())

    class T(Trainer):
        def forward(self, x, y, is_logging=False):
            loss = torch.nn.functional.mse_loss(self.model(x), y)
            return loss, {'loss': (loss, LogType.SCALAR)}

    net = _net().to(dev)
    data = _batches(STEPS)
    mine = [(x[rank * 2:rank * 2 + 2].clone(), y[rank * 2:rank * 2 + 2].clone()) for x, y in data]
    if rank == 1:
        mine[NAN_STEP - 1][0][0, 0, 0] = float('nan')                     # only rank 1 sees a NaN, through its data (replays included)
    opt = poptim.Adam(net.parameters(), lr=1e-2) if hip_adam else torch.optim.Adam(net.parameters(), lr=1e-2, fused=True)
    tr = T(net, opt, mine, mine[:1], max_step=STEPS, valid_max_step=1, save_interval=10 ** 6, log_interval=10 ** 6,
           save_dir=tmp, save_prefix='dp', seed=3)
    tr.graph_steps, tr.graph_warmup = graph, 1
    if clip:
        tr.grad_clip, tr.grad_norm = CLIP
    net.train()
    for i in range(1, STEPS + 1):
        tr.step = i
        tr.train(i)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in net.state_dict().items()}
    # the mode every captured step graph REALLY ran with (a fallback must be visible to the test), and the backend
    out['__modes__'] = np.asarray([str(v.ddp) for v in getattr(tr, '_graphs', {}).values() if v.captured])
    out['__backend__'] = np.asarray(dist.get_backend())
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


CLIP = (0.05, 0.2)          # Trainer.grad_clip, Trainer.grad_norm of the clipping variant: both bite on this problem


def _two_ranks(tmp_path, graph, hip_adam, ddp_mode, share, clip, expect_backend, expect_modes):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q, graph, hip_adam, ddp_mode, share, clip)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=400) for _ in procs)
    assert all(isinstance(v, dict) for v in res.values()), res
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for r in (0, 1):
        assert str(res[r].pop('__backend__')) == expect_backend
        modes = [str(m) for m in res[r].pop('__modes__')]
        assert modes == expect_modes, (r, modes)                          # what ran, not what was asked for
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k                    # ranks bit-identical
    # one process, full batches, the NaN step skipped by everybody
    net = _net().double()
    opt = torch.optim.Adam(net.parameters(), lr=1e-2)
    data = _batches(STEPS)
    for step in range(1, STEPS + 1):
        if step == NAN_STEP:
            continue
        x, y = data[step - 1]
        opt.zero_grad()
        torch.nn.functional.mse_loss(net(x.double()), y.double()).backward()
        if clip:                                                          # pytorch_sound/trainer.py:184-191
            for p in net.parameters():
                p.grad = p.grad.clamp(-CLIP[0], CLIP[0])
            torch.nn.utils.clip_grad_norm_(net.parameters(), CLIP[1])
        opt.step()
    for k, v in net.state_dict().items():
        assert np.abs(v.numpy() - res[0][k]).max() <= 2e-5 * max(1.0, np.abs(v.numpy()).max()), k


@pytest.mark.timeout(900)
@pytest.mark.parametrize('graph,hip_adam,ddp_mode,clip', [(True, True, None, False), (False, True, None, False), (True, False, None, False),
                                                          (True, True, 'events', False), (True, True, None, True),
                                                          (False, False, None, True)])
def test_two_ranks_on_one_gpu(tmp_path, graph, hip_adam, ddp_mode, clip):
    """two ranks share the one GPU over gloo: the default graph mode there is `deferred` - and so is `events`, which this HIP
    runtime cannot capture (asserted: the mode recorded by the step graph, not the one asked for).  clip: Trainer.grad_clip +
    grad_norm, folded into the HIP optimizer step (K18) or, with torch's fused Adam, the reference's per-parameter formulation -
    the global norm is taken over the AVERAGED gradients on every rank."""
    _two_ranks(tmp_path, graph, hip_adam, ddp_mode, True, clip, 'gloo', ['deferred'] if graph else [])


@pytest.mark.timeout(900)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='RCCL needs one device per rank: this box has one GPU (the captured-RCCL '
                    'path is covered there by the one-rank group of test_rccl_all_reduce_captured_in_the_step_graph)')
@pytest.mark.parametrize('graph', [True, False])
def test_two_ranks_rccl_captured_all_reduce(tmp_path, graph):
    """the same training over RCCL on two devices: the step graph must have run in `capture` mode (all-reduce of every bucket
    captured into the graph) on both ranks - runs wherever two GPUs are visible."""
    _two_ranks(tmp_path, graph, True, None, False, False, 'nccl', ['capture'] if graph else [])


# ---- graph mode: buckets are released INSIDE the replayed backward ------------------------------------------------------------
# The HIP runtime bundled with this torch (7.0) refuses external event-record nodes inside a capture (tools/probe_extevent_inproc.py;
# ROCm 7.2's accepts them, tools/mb/probe_extevent.hip), so FlatGradReducer.graph_mode() resolves to 'capture' under RCCL: the
# all-reduce of every bucket is captured INTO the step graph on RCCL's stream, forked right behind the bucket's last gradient
# and joined at the end of the backward.  Two ranks cannot share the test box's single GPU under RCCL, so the captured path is
# driven with a one-rank process group (PSND_DDP_FORCE=1): same code, same graph topology, the sum over one rank is the identity.
def _deep_net():
    torch.manual_seed(9)
    layers = []
    for i in range(10):
        layers += [torch.nn.Conv1d(64, 64, 5, padding=2), torch.nn.Tanh()]
    return torch.nn.Sequential(torch.nn.Conv1d(4, 64, 3, padding=1), *layers, torch.nn.Conv1d(64, 2, 1))


def _capture_worker(port, tmp, q, use_ddp):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK='0',
                          PSND_DDP_FORCE='1' if use_ddp else '0')
        os.environ.pop('PSND_DDP_GRAPH', None)
        import torch.distributed as dist
        from pytorch_sound_amd import optim as poptim
        from pytorch_sound_amd.trainer import Trainer, LogType
        if use_ddp:
            torch.cuda.set_device(0)
            dist.init_process_group('nccl', rank=0, world_size=1)
        dev = torch.device('cuda:0')

        class T(Trainer):
            def forward(self, x, y, is_logging=False):
                loss = torch.nn.functional.mse_loss(self.model(x), y)
                return loss, {'loss': (loss, LogType.SCALAR)}

        net = _deep_net().to(dev)
        g = torch.Generator().manual_seed(5)
        data = [(torch.randn(4, 4, 512, generator=g), torch.randn(4, 2, 512, generator=g)) for _ in range(6)]
        data[3][0][0, 0, 0] = float('nan')                          # step 4: the NaN flag rides in the last bucket, the step is skipped
        tr = T(net, poptim.Adam(net.parameters(), lr=1e-3), data, data[:1], max_step=6, valid_max_step=1, save_interval=10 ** 6,
               log_interval=10 ** 6, save_dir=tmp, save_prefix='cap' + str(int(use_ddp)), seed=3)
        info = {}
        if use_ddp:
            from pytorch_sound_amd import distributed as pdist
            assert tr._reducer is not None and tr._reducer.active
            tr._reducer.remove()
            tr._reducer = pdist.FlatGradReducer(net, bucket_bytes=64 << 10, force=True)
        tr.graph_steps, tr.graph_warmup = True, 1
        net.train()
        for i in range(1, 7):
            tr.step = i
            tr.train(i)
        torch.cuda.synchronize()
        if use_ddp:
            red = tr._reducer
            info = {'modes': [v.ddp for v in tr._graphs.values() if v.captured], 'emit': list(red.emit_log),
                    'nb': len(red.buckets), 'nparams': len(red.params), 'sizes': [len(b['params']) for b in red.buckets]}
            dist.destroy_process_group()
        q.put((use_ddp, info, {k: v.cpu().numpy() for k, v in net.state_dict().items()}))
    except Exception as e:
        q.put((use_ddp, repr(e)))
        raise


@pytest.mark.timeout(900)
def test_rccl_all_reduce_captured_in_the_step_graph(tmp_path):
    ctx = mp.get_context('spawn')
    res = {}
    for use_ddp in (False, True):
        q = ctx.Queue()
        p = ctx.Process(target=_capture_worker, args=(_port(), str(tmp_path), q, use_ddp))
        p.start()
        got = q.get(timeout=400)
        p.join(timeout=120)
        assert p.exitcode == 0 and len(got) == 3, got
        res[use_ddp] = got
    info = res[True][1]
    assert info['modes'] == ['capture'], info                            # no fallback happened
    nb = info['nb']
    assert nb >= 3
    # launch order inside the captured backward: the all-reduce of bucket i was enqueued (forked onto RCCL's stream) the moment its
    # last gradient existed - bucket 0 long before the last backward segment - and the buckets went out in fixed order
    assert [i for i, _ in info['emit']] == list(range(nb))
    arrived = [a for _, a in info['emit']]
    need = list(np.cumsum(info['sizes']))
    assert all(a >= n for a, n in zip(arrived, need)) and arrived == sorted(arrived), (arrived, need)
    assert arrived[nb // 2] <= need[nb // 2] + 4          # released as the gradients arrive, not at the end
    assert arrived[0] < info['nparams'] // 2
    for k in res[False][2]:
        # sum over one rank = identity: the same training, NaN step skipped in both (two processes: the convolution library may
        # pick other algorithms)
        assert np.isfinite(res[True][2][k]).all()
        assert np.allclose(res[False][2][k], res[True][2][k], rtol=1e-4, atol=1e-6), k


# ---- round 6: the kernels' own hand-over paths under a REAL two-rank sum ------------------------------------------------
# A small HiFi-GAN generator on the channels-last kernels - resblock branches on parallel streams, parameter-side backward on the parameter
# stream, gradients produced on several streams and handed to the reducer from hooks - trained by two ranks that share the GPU over gloo,
# each on its half of every batch: the ranks must end bit-identical, and equal (to the summation order of the weight-gradient slabs) to ONE
# process without a reducer on the full batches.  Eager (hook-overlapped all-reduce) and captured steps (deferred all-reduce under gloo).
def _gan_worker(rank, world, port, tmp, q, graph):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK=str(rank),
                          PSND_DIST_SHARE_GPU='1', PSND_LAB='1')
        os.environ.pop('PSND_DDP_GRAPH', None)
        import torch.distributed as dist
        from pytorch_sound_amd import distributed as pdist
        assert pdist.init_from_env('nccl') if world > 1 else True
        out = _gan_train(rank, world, tmp, graph)
        q.put((rank, out))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception as e:                                                # noqa: BLE001
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))
        raise


def _gan_train(rank, world, tmp, graph, steps=4):
    from test_gpu_branches import _gen
    from pytorch_sound_amd import cl, kernels as K, optim as poptim
    from pytorch_sound_amd.trainer import Trainer, LogType
    g = _gen(11)
    g.cl_branches = True
    cl.BRANCH_PARAM_GRADS = True

    class Step(Trainer):
        def forward(self, x, y, is_logging=False):
            loss = K.l1_loss(self.model(x), y)
            return loss, {'loss': (loss, LogType.SCALAR)}

    gen = torch.Generator().manual_seed(3)
    full = [(torch.randn(4, 80, 16, generator=gen), torch.randn(4, 1, 128, generator=gen)) for _ in range(steps)]
    n = 4 // world
    data = [(x[rank * n:(rank + 1) * n].cuda(), y[rank * n:(rank + 1) * n].cuda()) for x, y in full]
    tr = Step(g, poptim.Adam(g.parameters(), lr=1e-3), data, data[:1], max_step=steps, valid_max_step=1, save_interval=10 ** 6,
              log_interval=10 ** 6, save_dir=tmp, save_prefix='gan%d' % rank, seed=1)
    assert (tr._reducer is not None and tr._reducer.active) == (world > 1)
    tr.graph_steps, tr.graph_warmup = graph, 1
    g.train()
    for i in range(1, steps + 1):
        tr.step = i
        tr.train(i)
    torch.cuda.synchronize()
    out = {k: v.detach().float().cpu().numpy() for k, v in g.state_dict().items()}
    out['__modes__'] = np.asarray([str(v.ddp) for v in getattr(tr, '_graphs', {}).values() if v.captured])
    return out


@pytest.mark.timeout(900)
@pytest.mark.parametrize('graph', [False, True])
def test_two_ranks_hifigan_with_branches(tmp_path, graph):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_gan_worker, args=(r, 2, port, str(tmp_path), q, graph)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=400) for _ in procs)
    assert all(isinstance(v, dict) for v in res.values()), res
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    q1 = ctx.Queue()
    one = ctx.Process(target=_gan_worker, args=(0, 1, _port(), str(tmp_path), q1, graph))
    one.start()
    ref = q1.get(timeout=400)[1]
    one.join(timeout=120)
    assert isinstance(ref, dict), ref
    modes = [[str(m) for m in res[r].pop('__modes__')] for r in (0, 1)]
    ref.pop('__modes__')
    assert modes[0] == modes[1] == (['deferred'] if graph else []), modes
    worst = 0.0
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k                    # ranks bit-identical
        d = np.abs(res[0][k] - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-12)
        worst = max(worst, d)
    # Adam's first steps move every weight by ~lr whatever the gradient's size: a gradient that differs in the last bits moves the weight the
    # same way.  What this bounds is a LOST or doubled contribution (a bucket released early, a rank's half missing): that moves weights by
    # O(lr) = 1e-3 relative to weights of O(0.1 .. 1)
    assert worst <= 2e-4, worst
