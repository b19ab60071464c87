"""Look-ahead of an LR schedule (no GPU needed).

The reference's Trainer calls ``scheduler.step()`` after every SUCCESSFUL step (pytorch_sound/trainer.py:211-214): a skipped (NaN) step
does not advance the schedule.  On the device-skip path the host learns of a skip only a few steps later, so it cannot know which learning
rate the step it is enqueueing should use - but for every scheduler of ``torch.optim.lr_scheduler`` whose ``step()`` takes no argument the
rate after j successful steps is a pure function of j.  ``LookAhead`` runs a SHADOW of the user's scheduler ahead of the real one and hands
out row j = the rates of all parameter groups after j successful steps; the optimizer kernel picks the row by the count of steps that really
succeeded (``psnd_adam_step_sched``).  The real scheduler and optimizer are never touched by it.

The shadow is a shallow copy of the scheduler whose ``optimizer`` is a stand-in: copies of the ``param_groups`` without their parameters,
``_opt_called = True`` and a ``step`` marked ``_wrapped_by_lr_sched`` (torch's order-of-calls warnings stay quiet).  List and dict state is
deep-copied, ``lr_lambdas`` are shared (closures need not be copyable), the ``_schedulers`` of SequentialLR / ChainedScheduler are shadowed
recursively against the same stand-in.
"""
import copy
import inspect
import warnings

import torch
from torch.optim.lr_scheduler import LRScheduler


class _StandInOptimizer:
    """what a scheduler's step() needs of an optimizer: param_groups (no parameters in them) and the marks of torch's call-order check"""

    def __init__(self, optimizer):
        self.param_groups = [{k: copy.deepcopy(v) for k, v in g.items() if k != 'params'} for g in optimizer.param_groups]
        self.defaults = dict(getattr(optimizer, 'defaults', {}))
        self._opt_called = True

        def step(*args, **kwargs):
            raise RuntimeError('the stand-in optimizer of an LR look-ahead takes no steps')
        step._wrapped_by_lr_sched = True
        self.step = step


_SHARED = ('lr_lambdas',)        # callables of the user: shared with the real scheduler, never copied


def _shadow(scheduler, stand_in, seen):
    if id(scheduler) in seen:
        return seen[id(scheduler)]
    twin = copy.copy(scheduler)
    seen[id(scheduler)] = twin
    for k, v in scheduler.__dict__.items():
        if k == 'optimizer':
            twin.optimizer = stand_in
        elif k == '_schedulers':
            twin._schedulers = [_shadow(s, stand_in, seen) for s in v]
        elif k in _SHARED:
            twin.__dict__[k] = list(v) if isinstance(v, list) else v
        elif isinstance(v, (list, dict)):
            twin.__dict__[k] = copy.deepcopy(v)
    return twin


def shadow_of(scheduler):
    """(shadow scheduler, its stand-in optimizer) at the scheduler's present state"""
    stand_in = _StandInOptimizer(scheduler.optimizer)
    return _shadow(scheduler, stand_in, {}), stand_in


def _step_takes_no_argument(scheduler) -> bool:
    try:
        sig = inspect.signature(scheduler.step)
    except (TypeError, ValueError):
        return False
    return not any(p.default is p.empty and p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD, p.KEYWORD_ONLY) for p in sig.parameters.values())


def members(scheduler):
    yield scheduler
    for s in getattr(scheduler, '_schedulers', None) or ():
        yield from members(s)


def why_not_eligible(scheduler):
    """None when the schedule can be looked ahead, else the reason (a string)"""
    if not isinstance(scheduler, LRScheduler):
        return 'not a torch.optim.lr_scheduler.LRScheduler'
    for s in members(scheduler):
        if not isinstance(s, LRScheduler):
            return 'a member scheduler is not an LRScheduler'
        if not _step_takes_no_argument(s):
            return '%s.step() takes an argument (the schedule depends on more than the step count)' % type(s).__name__
    opt = getattr(scheduler, 'optimizer', None)
    groups = getattr(opt, 'param_groups', None)
    if not groups:
        return 'no optimizer attached'
    if any(isinstance(g.get('lr'), torch.Tensor) for g in groups):
        return 'a tensor learning rate (updated in place by the scheduler)'
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            twin, stand_in = shadow_of(scheduler)
            before = [{k: copy.deepcopy(v) for k, v in g.items() if k != 'lr'} for g in stand_in.param_groups]
            twin.step()
    except Exception as e:                                  # noqa: BLE001 - a scheduler the shadow cannot stand in for
        return 'its shadow cannot be stepped (%s)' % repr(e)[:120]
    after = [{k: v for k, v in g.items() if k != 'lr'} for g in stand_in.param_groups]
    if after != before:
        changed = sorted({k for a, b in zip(after, before) for k in set(a) | set(b) if a.get(k) != b.get(k)})
        return 'its step() rewrites %s of the parameter groups, not only lr' % ', '.join(changed)
    if not all(isinstance(g['lr'], (int, float)) for g in stand_in.param_groups):
        return 'its step() leaves a learning rate that is no number'
    return None


def eligible(scheduler) -> bool:
    return why_not_eligible(scheduler) is None


class LookAhead:
    """rows of the schedule ahead of the real scheduler: ``row(j)`` = [lr of every group] after j further successful steps, j = 0 being
    the rates the optimizer's groups hold now.  Rows are produced in order and remembered for ``keep`` indices back."""

    def __init__(self, scheduler, keep: int = 512):
        why = why_not_eligible(scheduler)
        if why is not None:
            raise ValueError('LR look-ahead: ' + why)
        self._twin, self._stand_in = shadow_of(scheduler)
        self._keep = int(keep)
        self._rows = {0: [float(g['lr']) for g in self._stand_in.param_groups]}
        self._last = 0
        self.n_groups = len(self._stand_in.param_groups)

    def row(self, j: int):
        if j < 0 or j <= self._last - self._keep:
            raise IndexError('LR look-ahead: row %d is no longer kept (at %d)' % (j, self._last))
        while self._last < j:
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                self._twin.step()
            self._last += 1
            self._rows[self._last] = [float(g['lr']) for g in self._stand_in.param_groups]
            self._rows.pop(self._last - self._keep, None)
        return self._rows[j]

    def rows(self, n: int):
        return [list(self.row(j)) for j in range(n)]
