"""Trainer with an LR scheduler on the device-skip / hipGraph path (`async_scheduler`): the learning rate of a step in flight is chosen on
the device by the count of steps that succeeded, the real scheduler is replayed as the flags reach the host.  Run A is that path, run B
(`async_nan_check = False`) the reference's synchronous loop: parameters, Adam state, scheduler state, learning rates and the NaN log lines
must be the same - with NaN losses at the first step, at two consecutive steps, at a step where StepLR(2, 0.5) changes the rate and at the
last step.  The poison comes from the data (a forward() that reads self.step is kept eager by graph_steps = 'auto')."""
import io
import logging
import math
import os
import re
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.optim import lr_scheduler as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 24
NAN_AT = (1, 4, 9, 10, 24)          # first / where StepLR(2, .5) steps the rate / two in a row / last


def _net(dev):
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 1)).to(dev)


def _batches(dev, nan_at=NAN_AT, n=STEPS):
    g = torch.Generator().manual_seed(5)
    out = []
    for i in range(1, n + 1):
        x, y = torch.randn(4, 8, generator=g), torch.randn(4, 1, generator=g)
        s = torch.tensor(float('nan') if i in nan_at else 1.0)
        out.append((x.to(dev), y.to(dev), s.to(dev)))
    return out


SCHEDULERS = {
    'StepLR': lambda o: S.StepLR(o, 2, 0.5),
    'ExponentialLR': lambda o: S.ExponentialLR(o, 0.9),
    'LambdaLR': lambda o: S.LambdaLR(o, lambda e: min(1.0, (e + 1) / 6.0) * math.sqrt(6.0 / max(6.0, e + 1.0))),   # Noam warm-up
    'SequentialLR': lambda o: S.SequentialLR(o, [S.LinearLR(o, start_factor=0.2, total_iters=5), S.ExponentialLR(o, 0.9)], milestones=[5]),
    'OneCycleLR': lambda o: S.OneCycleLR(o, max_lr=2e-2, total_steps=STEPS, cycle_momentum=False),
    # ends exactly where this run's 19 successful steps end: a look-ahead that counts skipped steps in flight as successes runs past it
    'OneCycleLR_short': lambda o: S.OneCycleLR(o, max_lr=2e-2, total_steps=STEPS - len(NAN_AT), cycle_momentum=False),
    'LambdaLR_negative': lambda o: S.LambdaLR(o, lambda e: 1.0 - 0.2 * e),                        # below zero after 6 successful steps
    'OneCycleLR_momentum': lambda o: S.OneCycleLR(o, max_lr=2e-2, total_steps=STEPS),             # rewrites betas: not eligible
}


def _optimizer(kind, net):
    from pytorch_sound_amd import optim as poptim
    if kind == 'stock':
        return torch.optim.Adam(net.parameters(), lr=1e-2)                # adopted by the Trainer, scheduler wrapper and all
    return poptim.AdamW([{'params': list(net[0].parameters()), 'lr': 1e-2}, {'params': list(net[2].parameters()), 'lr': 3e-3}],
                        weight_decay=0.01)


def _run(tmp, sched, opt_kind='stock', nan_at=NAN_AT, path='A', max_step=STEPS, save_interval=10 ** 6, lazy_host=False, edit_at=None,
         **attrs):
    """one Trainer.run(); path 'A': the defaults (must stay off the host check), 'B': async_nan_check = False"""
    from pytorch_sound_amd.trainer import Trainer, LogType
    from pytorch_sound_amd.utils.commons import LOGGER
    dev = torch.device('cuda:0')

    class T(Trainer):
        host_checks = 0
        block_polls = 0
        lr_seen = None

        def forward(self, x, y, s, is_logging=False):
            loss = F.mse_loss(self.model(x), y) * s
            return loss, {'loss': (loss, LogType.SCALAR)}

        def prepare(self, *inputs):
            if edit_at is not None and self.step == edit_at:
                self.optimizer.param_groups[0]['lr'] *= 0.1
            self.lr_seen.append(self.optimizer.param_groups[0]['lr'])
            return inputs

        def _loss_is_nan(self, loss):
            if path == 'A':
                raise AssertionError('the fast path waited for the host (_loss_is_nan)')
            self.host_checks += 1
            return super()._loss_is_nan(loss)

        def _poll_nan_log(self, block=False):
            if block:
                self.block_polls += 1
            elif lazy_host:
                return                                 # a host that never looks by itself: only the blocking catch-ups confirm steps
            return super()._poll_nan_log(block=block)

    net = _net(dev)
    data = _batches(dev, nan_at)
    clean = _batches(dev, ())[:1]
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        opt = _optimizer(opt_kind, net)
        sch = SCHEDULERS[sched](opt)
    buf = io.StringIO()
    hdl = logging.StreamHandler(buf)
    LOGGER.addHandler(hdl)
    try:
        tr = T(net, opt, data, clean, max_step=max_step, valid_max_step=1, save_interval=save_interval, log_interval=10 ** 6,
               save_dir=str(tmp), save_prefix='s', scheduler=sch, seed=1)
        tr.lr_seen = []
        if path not in ('A', 'A?'):
            tr.async_nan_check = False
        for k, v in attrs.items():
            setattr(tr, k, v)
        with warnings.catch_warnings():
            # torch's "scheduler before optimizer" checks must stay quiet on every path (the adopted optimizer keeps the tracking wrapper)
            warnings.filterwarnings('error', message=r'.*(Detected call of `lr_scheduler.step\(\)`|has been overridden after learning rate).*')
            tr.run()
        torch.cuda.synchronize()
    finally:
        LOGGER.removeHandler(hdl)
    text = buf.getvalue()
    return {'tr': tr, 'params': [p.detach().clone() for p in net.parameters()],
            'state': [{k: v.detach().clone() for k, v in opt.state[p].items()} for p in net.parameters()],
            'sched': sch.state_dict(), 'lrs': [g['lr'] for g in opt.param_groups], 'betas': [g['betas'] for g in opt.param_groups],
            'nan_lines': sorted(line for line in text.splitlines() if 'cur step NAN' in line), 'log': text}


def _same(a, b):
    for i, (p, q) in enumerate(zip(a['params'], b['params'])):
        assert torch.isfinite(p).all() and torch.equal(p, q), i
    for i, (s, t) in enumerate(zip(a['state'], b['state'])):
        assert sorted(s) == sorted(t) == ['exp_avg', 'exp_avg_sq', 'step']
        for k in s:
            assert torch.equal(s[k], t[k]), (i, k)
    assert a['sched'] == b['sched']
    assert a['lrs'] == b['lrs'] and a['betas'] == b['betas']
    assert a['nan_lines'] == b['nan_lines']


def _n_changes(seq):
    return sum(1 for u, v in zip(seq, seq[1:]) if u != v)


@pytest.fixture(scope='module')
def run_b(tmp_path_factory):
    """the synchronous runs, computed once per (scheduler, optimizer) and left unchanged"""
    cache = {}

    def get(sched, opt_kind):
        if (sched, opt_kind) not in cache:
            cache[(sched, opt_kind)] = _run(tmp_path_factory.mktemp('b'), sched, opt_kind, path='B')
        return cache[(sched, opt_kind)]
    return get


@pytest.mark.parametrize('opt_kind', ['stock', 'own'])
@pytest.mark.parametrize('sched', ['StepLR', 'ExponentialLR', 'LambdaLR', 'SequentialLR', 'OneCycleLR'])
def test_fast_path_with_a_scheduler_equals_the_synchronous_loop(tmp_path, run_b, sched, opt_kind):
    from pytorch_sound_amd import optim as poptim
    a = _run(tmp_path, sched, opt_kind)                    # raises if the host check runs
    b = run_b(sched, opt_kind)
    # A really is the fast path: the step was captured, no host check (this is what fails without the feature)
    assert 'captured the training step as a hipGraph' in a['log']
    assert a['tr']._lr_state is not None and int(a['tr']._lr_state.count.item()) == STEPS - len(NAN_AT)
    assert isinstance(a['tr'].optimizer, poptim.Adam) and isinstance(b['tr'].optimizer, poptim.Adam)
    assert getattr(a['tr'].optimizer.step, '_wrapped_by_lr_sched', False)
    assert b['tr'].host_checks == STEPS and 'hipGraph' not in b['log']
    _same(a, b)
    assert len(a['nan_lines']) == len(NAN_AT)
    for k in NAN_AT:
        assert any(re.search(r'\b%d cur step NAN is occured' % k, line) for line in a['nan_lines']), k
    assert a['sched']['last_epoch'] == STEPS - len(NAN_AT)
    # not vacuous: the rate moved, and the NaNs matter
    assert _n_changes(b['tr'].lr_seen) >= 3
    clean = _run(tmp_path / 'clean', sched, opt_kind, nan_at=(), path='B')
    assert clean['sched']['last_epoch'] == STEPS and clean['lrs'] != b['lrs']
    assert not torch.equal(clean['params'][0], b['params'][0])


@pytest.mark.parametrize('ring', [8, 256])
def test_a_host_that_lags_catches_up_by_blocking(tmp_path, run_b, ring):
    """no step is confirmed unless the Trainer blocks for it: with 8 rows it must (6 steps in flight), with 256 the whole run is in flight
    until run() ends - rows for every count of successes a step might see are in the ring"""
    a = _run(tmp_path, 'StepLR', 'own', lazy_host=True, _LR_RING=ring)
    _same(a, run_b('StepLR', 'own'))
    assert a['tr'].block_polls >= (4 if ring == 8 else 1)
    assert a['tr']._lr_state.ring.shape == (ring, 2)


def test_look_ahead_past_the_end_of_a_schedule(tmp_path):
    """OneCycleLR raises when stepped past total_steps.  The run itself never does (19 successes), but with the whole run in flight the
    row for `launched` successes is asked for: the Trainer catches up, starts a new shadow from the real scheduler and goes on"""
    a = _run(tmp_path / 'a', 'OneCycleLR_short', 'own', lazy_host=True)
    b = _run(tmp_path / 'b', 'OneCycleLR_short', 'own', path='B')
    _same(a, b)
    assert a['sched']['last_epoch'] == STEPS - len(NAN_AT) == a['sched']['total_steps']
    assert a['tr'].block_polls >= 2                        # the catch-up at the schedule's end, and the one that ends run()


def test_a_rate_the_optimizer_refuses_is_refused_before_it_reaches_the_ring(tmp_path):
    with pytest.raises(ValueError, match='finite rates >= 0'):
        _run(tmp_path, 'LambdaLR_negative', 'own')
    torch.cuda.synchronize()


def test_an_error_of_the_users_schedule_goes_up_as_it_is(tmp_path):
    def bad(e):
        if e >= 5:
            raise ValueError('the recipe\'s lambda gave up')
        return 1.0
    SCHEDULERS['LambdaLR_raises'] = lambda o: S.LambdaLR(o, bad)
    try:
        with pytest.raises(ValueError, match='gave up'):
            _run(tmp_path, 'LambdaLR_raises', 'own')
    finally:
        del SCHEDULERS['LambdaLR_raises']
    torch.cuda.synchronize()


def test_checkpoint_and_resume(tmp_path):
    got = {}
    for path in ('A', 'B'):
        d = tmp_path / path
        first = _run(d, 'StepLR', 'stock', path=path, max_step=12, save_interval=12)
        ck = torch.load(str(d / 'models' / 's' / 'Sequential' / 'step_000012.chkpt'), map_location='cpu', weights_only=False)
        second = _run(d, 'StepLR', 'stock', path=path, max_step=STEPS, save_interval=12)
        assert 'previous step=12' in second['log']
        got[path] = (first, ck, second)
    (a1, cka, a2), (b1, ckb, b2) = got['A'], got['B']
    assert cka['scheduler'] == ckb['scheduler'] and cka['scheduler']['last_epoch'] == 12 - 4          # steps 1, 4, 9, 10 skipped
    assert cka['optim']['param_groups'] == ckb['optim']['param_groups']
    for k in cka['model']:
        assert torch.equal(cka['model'][k], ckb['model'][k]), k
    _same(a1, b1)
    _same(a2, b2)
    assert 'captured the training step as a hipGraph' in a2['log']


@pytest.mark.parametrize('edit_at,how', [(9, {}),
                                         # the edit at a logging step (9: also a NaN step): its catch-up comes between the edit and the
                                         # launch.  lazy_host: steps are certainly still in flight then, whatever the GPU's pace
                                         (9, {'log_interval': 3, 'lazy_host': True}),
                                         (6, {'log_interval': 3, 'lazy_host': True}),
                                         (6, {'log_interval': 3}),
                                         (9, {'lazy_host': True, '_NAN_RING': 6})],      # the catch-up of a full flag ring sees it first
                         ids=['plain', 'logging_nan_step', 'logging_step', 'logging_step_eager_host', 'flag_ring_full'])
def test_learning_rate_edited_by_hand_between_steps(tmp_path, edit_at, how):
    """`param_groups[0]['lr'] *= 0.1` from prepare(): the edit holds from that step on, as on the synchronous path - also when a blocking
    catch-up (a logging step, a full flag ring) replays scheduler steps on top of the edit before the next launch is staged: the rates the
    device goes on with, the scheduler's state and the groups' rates must not part ways.  (StepLR(2, 0.5): a factor of 0.1 and the
    halvings commute exactly, so the steps in flight at the edit do not show.)"""
    how = dict(how)
    sched = 'StepLR'
    a = _run(tmp_path / 'a', sched, 'own', edit_at=edit_at, **how)
    how.pop('lazy_host', None)
    b = _run(tmp_path / 'b', sched, 'own', edit_at=edit_at, path='B', **how)
    _same(a, b)
    plain = _run(tmp_path / 'p', sched, 'own', path='B', **how)
    assert b['lrs'][0] == pytest.approx(0.1 * plain['lrs'][0], rel=1e-12) and b['lrs'][1] == plain['lrs'][1]
    assert not torch.equal(b['params'][0], plain['params'][0])
    assert a['sched']['_last_lr'] == b['sched']['_last_lr'] == b['lrs']         # what a checkpoint would carry is what the run trained with


@pytest.mark.parametrize('case', ['momentum_cycling', 'switched_off'])
def test_what_cannot_ride_along_keeps_the_synchronous_path(tmp_path, case):
    sched = 'OneCycleLR_momentum' if case == 'momentum_cycling' else 'StepLR'
    attrs = {} if case == 'momentum_cycling' else {'async_scheduler': False}
    a = _run(tmp_path / 'a', sched, 'stock', path='A?', **attrs)            # the defaults otherwise; the host check is allowed (and counted)
    b = _run(tmp_path / 'b', sched, 'stock', path='B')
    assert a['tr'].host_checks == STEPS == b['tr'].host_checks
    assert a['tr']._lr_state is None and 'hipGraph' not in a['log']
    _same(a, b)
    if case == 'momentum_cycling':
        assert a['betas'][0][0] != 0.9                                      # the scheduler did cycle the momentum


# ---- two ranks sharing the one GPU over gloo: a NaN on one rank only - both skip, both schedules stand still for that step -----------------
DDP_STEPS, DDP_NAN = 9, 5


def _ddp_worker(rank, world, port, tmp, q):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK=str(rank),
                          PSND_DIST_SHARE_GPU='1')
        os.environ.pop('PSND_DDP_GRAPH', None)
        import torch.distributed as dist
        from pytorch_sound_amd import distributed as pdist, optim as poptim
        from pytorch_sound_amd.trainer import Trainer, LogType
        assert pdist.init_from_env('nccl')                                    # share mode switches to gloo itself
        dev = torch.device('cuda', torch.cuda.current_device())

        class T(Trainer):
            def forward(self, x, y, s, is_logging=False):
                loss = F.mse_loss(self.model(x), y) * s
                return loss, {'loss': (loss, LogType.SCALAR)}

            def _loss_is_nan(self, loss):
                raise AssertionError('the fast path waited for the host (_loss_is_nan)')

        net = _net(dev)
        data = _batches(dev, (DDP_NAN,) if rank == 1 else (), DDP_STEPS)
        mine = [(x[rank * 2:rank * 2 + 2].clone(), y[rank * 2:rank * 2 + 2].clone(), s) for x, y, s in data]
        opt = poptim.Adam(net.parameters(), lr=1e-2)
        sch = S.StepLR(opt, 2, 0.5)
        tr = T(net, opt, mine, mine[:1], max_step=DDP_STEPS, valid_max_step=1, save_interval=10 ** 6, log_interval=10 ** 6,
               save_dir=tmp, save_prefix='dp%d' % rank, scheduler=sch, seed=3)
        tr.graph_steps, tr.graph_warmup = True, 1
        tr.run()
        torch.cuda.synchronize()
        out = {'params': [p.detach().cpu().numpy() for p in net.parameters()], 'sched': sch.state_dict(), 'lr': opt.param_groups[0]['lr'],     # (numpy: pickled by value)
               'count': int(tr._lr_state.count.item()), 'graphs': sum(1 for v in tr._graphs.values() if v.captured),
               'steps': [float(opt.state[p]['step']) for p in net.parameters()]}
        q.put((rank, out))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                                    # the parent must not wait for its timeout
        import traceback
        q.put((rank, repr(e) + traceback.format_exc()))
        raise


@pytest.mark.timeout(900)
def test_two_ranks_skip_together_and_their_schedules_agree(tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_dist_share import _port
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=400) for _ in procs)
    assert all(isinstance(v, dict) for v in res.values()), res
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    r0, r1 = res[0], res[1]
    for p, q_ in zip(r0['params'], r1['params']):
        assert np.isfinite(p).all() and np.array_equal(p, q_)
    assert r0['sched'] == r1['sched'] and r0['sched']['last_epoch'] == DDP_STEPS - 1
    assert r0['lr'] == r1['lr'] == 1e-2 * 0.5 ** ((DDP_STEPS - 1) // 2)
    assert r0['count'] == r1['count'] == DDP_STEPS - 1
    assert r0['steps'] == r1['steps'] == [float(DDP_STEPS - 1)] * 4
    assert r0['graphs'] == r1['graphs'] == 1
