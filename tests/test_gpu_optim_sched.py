"""psnd_adam_step_sched through `optimizer.lr_ahead` (kernel level): the learning rate of every launch is read on the device from the
ring row of the steps that succeeded so far, and the last group's launch counts a step that was not skipped.  Against the SAME optimizer
stepped with `group['lr']` set on the host to that row and the same `found_inf`: parameters, exp_avg, exp_avg_sq and step bit-equal,
the device counter = the number of successes.  Tensors at the edges of the 2048-element chunk, one off a 16-byte boundary, two groups,
a ring of 4 rows over 12 steps (the index wraps), Adam and AdamW, with and without the fused clip."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')

SIZES = (1, 2047, 2048, 2049, 5000)
FLAGS = [0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0]           # found_inf per step: 8 successes over a ring of 4 rows
ROWS = 4


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    out = [torch.randn(n, generator=g) for n in SIZES]
    out.append(torch.randn(3, 700, generator=g))       # placed 4 bytes off a 16-byte boundary below
    return out


def _on_device(ts):
    dev = []
    for i, t in enumerate(ts):
        if i == len(ts) - 1:
            base = torch.empty(t.numel() + 1, device=DEV)
            assert base.data_ptr() % 16 == 0
            base[1:] = t.flatten().to(DEV)
            d = base[1:].view(t.shape)
            assert d.data_ptr() % 16 == 4
        else:
            d = t.to(DEV)
        dev.append(d.requires_grad_(True))
    return dev


def _schedule(j):
    """the rates of the two groups after j successes: nothing a float holds exactly, different per group"""
    return [1e-2 * 0.83 ** j, 3e-3 / (1.0 + 0.37 * j)]


def _make(cls, seed):
    ps = _on_device(_tensors(seed))
    opt = cls([{'params': ps[:3]}, {'params': ps[3:], 'weight_decay': 0.05, 'betas': (0.8, 0.99)}], lr=1.0, weight_decay=0.01)
    return ps, opt


def _grads(seed, step):
    g = torch.Generator().manual_seed(1000 * seed + step)
    return [3.0 * torch.randn(n, generator=g) for n in SIZES] + [3.0 * torch.randn(3, 700, generator=g)]


@pytest.mark.parametrize('clip', [None, (0.5, 2.0)], ids=['noclip', 'fused_clip'])
@pytest.mark.parametrize('kind', ['Adam', 'AdamW'])
def test_lr_chosen_on_the_device_equals_lr_set_on_the_host(kind, clip):
    from pytorch_sound_amd import optim as poptim
    cls = getattr(poptim, kind)
    assert cls._supports_lr_ahead is True
    pa, oa = _make(cls, 1)
    pb, ob = _make(cls, 1)
    ring = torch.zeros((ROWS, 2), dtype=torch.float32).pin_memory()
    count = torch.zeros((), dtype=torch.int32, device=DEV)
    good = 0
    for step, bad in enumerate(FLAGS):
        flag = torch.full((), float(bad), device=DEV)
        grads = _grads(1, step)
        for p, q, g in zip(pa, pb, grads):
            p.grad = g.to(DEV)
            q.grad = g.to(DEV)
        # A: the host does not know `good`; it provides every row this launch could read (here: the one row, the run is synchronous)
        torch.cuda.synchronize()                       # the ring row being replaced is no longer read
        ring[good % ROWS] = torch.tensor(_schedule(good), dtype=torch.float64)
        oa.found_inf, oa.lr_ahead = flag, (ring, ROWS, count)
        # B: the rate on the host
        for grp, lr in zip(ob.param_groups, _schedule(good)):
            grp['lr'] = lr
        ob.found_inf = flag
        if clip is not None:
            oa.fused_clip = ob.fused_clip = clip
        oa.step()
        ob.step()
        assert oa.lr_ahead_used
        del oa.found_inf, oa.lr_ahead, ob.found_inf
        if clip is not None:
            del oa.fused_clip, ob.fused_clip
        good += 0 if bad else 1
        assert int(count.item()) == good, step
        for grp in oa.param_groups:
            assert grp['lr'] == 1.0                    # never read, never written
    assert good == 8 > ROWS
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert torch.isfinite(p).all()
        assert torch.equal(p.detach(), q.detach()), i
        for k in ('exp_avg', 'exp_avg_sq', 'step'):
            assert torch.equal(oa.state[p][k], ob.state[q][k]), (i, k)
        assert float(oa.state[p]['step']) == good
    # not vacuous: the same gradients under the FIRST row only end elsewhere
    pc, oc = _make(cls, 1)
    for grp, lr in zip(oc.param_groups, _schedule(0)):
        grp['lr'] = lr
    for step, bad in enumerate(FLAGS):
        for p, g in zip(pc, _grads(1, step)):
            p.grad = g.to(DEV)
        oc.found_inf = torch.full((), float(bad), device=DEV)
        oc.step()
    assert not torch.equal(pc[1].detach(), pa[1].detach()) and not torch.equal(pc[4].detach(), pa[4].detach())


def test_only_the_last_launch_of_a_step_counts_it_and_a_skip_reads_nothing():
    from pytorch_sound_amd import optim as poptim
    ps, opt = _make(poptim.Adam, 2)
    ring = torch.full((ROWS, 2), float('nan'), dtype=torch.float32).pin_memory()      # a skipped step must not look at it
    count = torch.full((), 5, dtype=torch.int32, device=DEV)
    before = [p.detach().clone() for p in ps]
    for p, g in zip(ps, _grads(2, 0)):
        p.grad = g.to(DEV)
    opt.found_inf, opt.lr_ahead = torch.ones((), device=DEV), (ring, ROWS, count)
    opt.step()
    assert int(count.item()) == 5
    for p, b in zip(ps, before):
        assert torch.equal(p.detach(), b)
    # one group without gradients: the launch of the last group WITH work counts the step, once
    ring[1] = torch.tensor([1e-3, 2e-3])               # 5 % 4
    for p in ps[3:]:
        p.grad = None
    opt.found_inf = torch.zeros((), device=DEV)
    opt.step()
    assert int(count.item()) == 6
    assert all(torch.isfinite(p).all() for p in ps) and not torch.equal(ps[0].detach(), before[0]) and torch.equal(ps[4].detach(), before[4])
    del opt.found_inf, opt.lr_ahead


def test_protocol_refuses_a_ring_the_device_cannot_read():
    from pytorch_sound_amd import optim as poptim, _lib
    ps, opt = _make(poptim.Adam, 3)
    for p, g in zip(ps, _grads(3, 0)):
        p.grad = g.to(DEV)
    count = torch.zeros((), dtype=torch.int32, device=DEV)
    for ring, cnt in ((torch.zeros(ROWS, 2), count),                                              # pageable
                      (torch.zeros((ROWS, 1)).pin_memory(), count),                               # too few columns for two groups
                      (torch.zeros((ROWS, 2)).pin_memory(), torch.zeros((), dtype=torch.int64, device=DEV))):
        opt.lr_ahead = (ring, ROWS, cnt)
        with pytest.raises(_lib.PsndError):
            opt.step()
    del opt.lr_ahead
