"""Trainer with part of the model frozen, thawed or switched to eval() - from the start and BETWEEN two steps of a run whose steps are
captured (graph_steps = 'auto', the default).  A captured step repeats what Python decided at capture time, so the Trainer keys its graphs on
trainer.model_fingerprint() as well as on the batch signature: after a toggle the steps warm up and are captured again.

Every scenario runs three ways - 'auto', graph_steps = False, and a plain float64 torch.optim.Adam loop with the same toggles - on the
little net of test_gpu_auto_graph.py; the second model is made of this library's nodes (PointwiseFeedForward with dropout 0.1: its
train / eval flag changes the arithmetic), has no float64 twin and is compared 'auto' against eager, as test_gpu_dropout.py does.
Bounds: those of test_pure_forward_is_captured_by_default_and_trains_like_eager (1e-5 against eager, 2e-5 against float64)."""
import io
import logging
import os
import sys
import tempfile

import pytest
import torch
import torch.nn.functional as F

from test_gpu_auto_graph import _net, _data, _captured

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 16
TOGGLE_AT = 8               # between step 7 and step 8: steps 1-3 warm up, step 4 captures, 5-7 replay
CAPTURED = 'captured the training step'


def _ff_net():
    from pytorch_sound_amd.models.modules import PointwiseFeedForward
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Conv1d(4, 64, 1), PointwiseFeedForward(64, 0.1), torch.nn.Conv1d(64, 2, 1)).cuda()


def _freeze(*names):
    def f(net, tr=None):
        for n in names:
            net.get_parameter(n).requires_grad_(False)
    return f


def _thaw(*names):
    def f(net, tr=None):
        for n in names:
            net.get_parameter(n).requires_grad_(True)
    return f


def _eval_block(net, tr=None):
    net[1].eval()


def _run(make, mode, start=None, toggle=None, only_trainable=False, log_interval=10 ** 6, sched=False, clip=(0.0, 0.0)):
    """STEPS calls of Trainer.train(); `start(net)` before the Trainer is built, `toggle(net, trainer)` between step TOGGLE_AT - 1 and TOGGLE_AT"""
    from pytorch_sound_amd.trainer import Trainer, LogType
    from pytorch_sound_amd.utils.commons import LOGGER

    class T(Trainer):
        def forward(self, x, y, is_logging=False):
            loss = F.mse_loss(self.model(x), y)
            return loss, {'loss': (loss.detach(), LogType.SCALAR)}

    net = make()
    if start is not None:
        start(net)
    data = _data(STEPS)
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad or not only_trainable], lr=1e-2)
    sch = torch.optim.lr_scheduler.StepLR(opt, 4, 0.5) if sched else None
    buf = io.StringIO()
    hdl = logging.StreamHandler(buf)
    LOGGER.addHandler(hdl)
    try:
        tr = T(net, opt, data, data[:1], max_step=STEPS, valid_max_step=1, save_interval=10 ** 6, log_interval=log_interval,
               save_dir=tempfile.mkdtemp(prefix='psnd_frozen_'), grad_clip=clip[0], grad_norm=clip[1], scheduler=sch, seed=1)
        tr.graph_steps = mode
        net.train()
        held = {}                                                # name -> value at the moment it was frozen
        grads_none = True
        for i in range(1, STEPS + 1):
            if i == TOGGLE_AT and toggle is not None:
                toggle(net, tr)
            for k, p in net.named_parameters():
                if not p.requires_grad and k not in held:
                    held[k] = p.detach().clone()
                elif p.requires_grad:
                    held.pop(k, None)
            tr.step = i
            tr.train(i)
            grads_none = grads_none and all(p.grad is None for p in net.parameters() if not p.requires_grad)
        tr.sync_scheduler()
        torch.cuda.synchronize()
    finally:
        LOGGER.removeHandler(hdl)
    assert grads_none, 'a parameter with requires_grad == False had a gradient after a train() call'
    for k, v in held.items():
        assert torch.equal(net.get_parameter(k).detach(), v), 'frozen parameter %s moved' % k
    norm = getattr(tr.optimizer, 'last_grad_norm', None)
    return {'tr': tr, 'w': {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}, 'log': buf.getvalue(), 'held': sorted(held),
            'norm': None if norm is None else float(norm), 'lr': opt.param_groups[0]['lr']}


def _run64(start=None, toggle=None, sched=False, clip=(0.0, 0.0)):
    """the same run as a plain float64 loop: torch.optim.Adam, Trainer.clip_grad's two steps, the scheduler after every step"""
    ref = _net().double()
    if start is not None:
        start(ref)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-2)
    sch = torch.optim.lr_scheduler.StepLR(opt, 4, 0.5) if sched else None
    norm = None
    for i, (x, y) in enumerate(_data(STEPS), 1):
        if i == TOGGLE_AT and toggle is not None:
            toggle(ref)
        opt.zero_grad()
        F.mse_loss(ref(x.double()), y.double()).backward()
        if clip[0]:
            for p in ref.parameters():
                if p.grad is not None:
                    p.grad.clamp_(-clip[0], clip[0])
        if clip[1]:
            norm = float(torch.nn.utils.clip_grad_norm_([p for p in ref.parameters() if p.requires_grad], clip[1]))
        opt.step()
        if sch is not None:
            sch.step()
    return {'w': {k: v.detach().cpu() for k, v in ref.state_dict().items()}, 'norm': norm, 'lr': opt.param_groups[0]['lr']}


def _close(a, b, tol, what):
    errs = {k: float((a[k].double() - b[k].double()).abs().max()) / max(1.0, float(b[k].abs().max())) for k in b}
    worst = max(errs, key=errs.get)
    print('%s: worst %s %.1e (bound %.0e)' % (what, worst, errs[worst], tol))
    for k in b:
        assert errs[k] <= tol, (what, k, errs[k])


def _three_ways(make, twin=True, recapture=True, **kw):
    """'auto' against eager (1e-5) and against float64 (2e-5); with a toggle: captured before it, captured again after it"""
    auto = _run(make, 'auto', **kw)
    eager = _run(make, False, **kw)
    assert not _captured(eager['tr']) and CAPTURED not in eager['log']
    assert auto['held'] == eager['held']
    _close(auto['w'], eager['w'], 1e-5, 'auto / eager')
    assert auto['tr']._graph_auto_ok is True and _captured(auto['tr']), 'the run is captured at its end: a toggle does not switch auto off'
    n = auto['log'].count(CAPTURED)
    assert n == (2 if recapture else 1), '%d capture lines for the one batch signature\n%s' % (n, auto['log'])
    if twin:
        kw.pop('only_trainable', None), kw.pop('log_interval', None)
        ref = _run64(**kw)
        _close(auto['w'], ref['w'], 2e-5, 'auto / float64')
        _close(eager['w'], ref['w'], 2e-5, 'eager / float64')
        return auto, eager, ref
    return auto, eager, None


MODELS = [pytest.param(_net, True, id='torch_net'), pytest.param(_ff_net, False, id='ffn_dropout')]


# ---- (a) frozen from the start -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('only_trainable', [False, True], ids=['opt_all', 'opt_trainable'])
@pytest.mark.parametrize('make,twin', MODELS)
def test_frozen_from_the_start(make, twin, only_trainable):
    auto, _, _ = _three_ways(make, twin, recapture=False, start=_freeze('0.weight', '2.bias'), only_trainable=only_trainable)
    assert auto['held'] == ['0.weight', '2.bias']


def test_frozen_from_the_start_fused_clip_norm_is_over_the_trainable_parameters():
    """grad_clip and grad_norm with an optimizer over the trainable parameters only: the clip runs inside the optimizer launch and its norm
    (optimizer.last_grad_norm, of the last step) is clip_grad_norm_'s of the float64 twin.  Bound of the norm: the weights agree to 2e-5
    and the gradient of this net is Lipschitz in them with a constant of order one; fp32 rounding of a 256-element mean adds ~1e-6 - five times
    the weights' bound, relative."""
    clip = (0.05, 0.1)
    auto, eager, ref = _three_ways(_net, True, recapture=False, start=_freeze('0.weight', '2.bias'), only_trainable=True, clip=clip)
    for r in (auto, eager):
        assert r['norm'] is not None, 'the fused clip ran (optimizer and model agree on the trainable set)'
        assert abs(r['norm'] - ref['norm']) <= 1e-4 * ref['norm'], (r['norm'], ref['norm'])
    full = _run64(clip=clip)                                     # (the norm over ALL parameters is another number)
    assert abs(full['norm'] - ref['norm']) > 1e-2 * ref['norm']


# ---- (b) freeze, (c) unfreeze after the capture -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('make,twin,name', [pytest.param(_net, True, '2.weight', id='torch_net'),
                                            pytest.param(_ff_net, False, '1.ff.0.weight', id='ffn_dropout')])
def test_freeze_after_the_capture(make, twin, name):
    auto, _, _ = _three_ways(make, twin, toggle=_freeze(name))
    assert auto['held'] == [name]


@pytest.mark.parametrize('make,twin,name', [pytest.param(_net, True, '0.weight', id='torch_net'),
                                            pytest.param(_ff_net, False, '1.ff.2.weight', id='ffn_dropout')])
def test_unfreeze_after_the_capture(make, twin, name):
    auto, _, _ = _three_ways(make, twin, start=_freeze(name, '2.bias'), toggle=_thaw(name))
    assert auto['held'] == ['2.bias']
    start = make().state_dict()[name].cpu()
    assert float((auto['w'][name] - start).abs().max()) > 1e-3, 'the thawed parameter trains'


# ---- (d) eval() on a submodule ----------------------------------------------------------------------------------------------------------------
def test_eval_on_a_submodule_after_the_capture():
    """the feed-forward block's dropout goes off at step 8: replayed steps must stop dropping as the eager loop does"""
    auto, eager, _ = _three_ways(_ff_net, False, toggle=_eval_block)
    on = _run(_ff_net, False)                                    # dropout left on: another trajectory, so the comparison above can fail
    worst = max(float((on['w'][k] - eager['w'][k]).abs().max() / max(1.0, float(eager['w'][k].abs().max()))) for k in on['w'])
    assert worst > 1e-4, worst


# ---- (e) eager logging steps in between, (f) with a scheduler ----------------------------------------------------------------------------
@pytest.mark.parametrize('make,twin,name', [pytest.param(_net, True, '2.weight', id='torch_net'),
                                            pytest.param(_ff_net, False, '1.ff.0.weight', id='ffn_dropout')])
def test_freeze_after_the_capture_with_logging_steps(make, twin, name):
    """log_interval = 5: steps 5, 10 and 15 run eagerly between the replays (the second capture is step 12)"""
    _three_ways(make, twin, toggle=_freeze(name), log_interval=5)


def test_freeze_after_the_capture_with_a_scheduler():
    """StepLR on the lr_ahead path: the rate of a replayed step is chosen on the device, the schedule does not restart with the capture"""
    auto, eager, ref = _three_ways(_net, True, toggle=_freeze('2.weight'), sched=True)
    assert auto['lr'] == eager['lr'] == ref['lr'] == 1e-2 * 0.5 ** (STEPS // 4)


def test_reset_graphs_on_request():
    """an edit the fingerprint cannot see: the caller asks, the step is captured again and the run goes on as before"""
    plain = _run(_net, 'auto')
    seen = []

    def ask(net, tr):
        seen.append(_captured(tr))
        tr.reset_graphs()
        seen.append(_captured(tr))
    again = _run(_net, 'auto', toggle=ask)
    assert seen == [True, False]
    assert plain['log'].count(CAPTURED) == 1 and again['log'].count(CAPTURED) == 2 and _captured(again['tr'])
    _close(again['w'], plain['w'], 1e-5, 'with / without reset_graphs')


# ---- with a gradient reducer: a one-rank forced group ------------------------------------------------------------------------------------
def _ddp_worker(port, tmp, q, graph):
    try:
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        os.environ.update(RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK='0', PSND_DDP_FORCE='1')
        os.environ.pop('PSND_DDP_GRAPH', None)
        import torch.distributed as dist
        from pytorch_sound_amd._lib import PsndError
        from pytorch_sound_amd.trainer import Trainer, LogType
        torch.cuda.set_device(0)
        dist.init_process_group('nccl', rank=0, world_size=1)

        class T(Trainer):
            def forward(self, x, y, is_logging=False):
                loss = F.mse_loss(self.model(x), y)
                return loss, {'loss': (loss.detach(), LogType.SCALAR)}

        net = _net()
        _freeze('0.weight', '2.bias')(net)
        start = {k: v.detach().clone() for k, v in net.state_dict().items()}
        data = _data(STEPS)
        tr = T(net, torch.optim.Adam(net.parameters(), lr=1e-2), data, data[:1], max_step=STEPS, valid_max_step=1, save_interval=10 ** 6,
               log_interval=10 ** 6, save_dir=tmp, seed=1)
        assert tr._reducer is not None and tr._reducer.active and len(tr._reducer.params) == 2
        tr.graph_steps = graph
        net.train()
        none_ok = True
        for i in range(1, STEPS + 1):
            tr.step = i
            tr.train(i)
            none_ok = none_ok and all(p.grad is None for p in net.parameters() if not p.requires_grad)
        torch.cuda.synchronize()
        out = {'w': {k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}, 'none_ok': none_ok, 'captured': _captured(tr),
               'held': all(torch.equal(net.state_dict()[k], start[k]) for k in ('0.weight', '2.bias'))}
        net[0].bias.requires_grad_(False)                        # a toggle after construction: the reducer refuses the next step
        try:
            tr.train(STEPS + 1)
            out['error'] = None
        except PsndError as e:
            out['error'] = str(e)
        torch.cuda.synchronize()
        q.put(out)
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:                                       # the parent must not wait for its timeout
        import traceback
        q.put(repr(e) + traceback.format_exc())
        raise


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_one_rank_forced_group_with_frozen_parameters(tmp_path, graph):
    """FlatGradReducer over a one-rank RCCL group (the sum over one rank is the identity): parameters frozen before construction have no
    slot and stay untouched, the rest trains like the float64 loop; a toggle after construction raises"""
    import torch.multiprocessing as mp
    from test_gpu_dist_share import _port
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    p = ctx.Process(target=_ddp_worker, args=(_port(), str(tmp_path), q, graph))
    p.start()
    out = q.get(timeout=200)
    p.join(timeout=60)
    assert isinstance(out, dict), out
    assert p.exitcode == 0
    assert out['none_ok'] and out['held'] and out['captured'] == graph
    ref = _run64(start=_freeze('0.weight', '2.bias'))
    _close({k: torch.from_numpy(v) for k, v in out['w'].items()}, ref['w'], 2e-5, 'reducer / float64')
    assert out['error'] is not None and 'FlatGradReducer' in out['error'] and '2 parameters' in out['error'] and '1 do now' in out['error']
