"""trainer.model_fingerprint and Trainer.reset_graphs on the host: a captured training step is keyed on the batch signature AND on the
`requires_grad` bit of every parameter / the `training` bit of every module - each kind of toggle changes the fingerprint, nothing else does,
and a change drops the captured steps, clears the gradients of frozen parameters and the optimizer-coverage cache."""
import tempfile

import torch
import torch.nn as nn

from pytorch_sound_amd.trainer import CapturedStep, Trainer, LogType, model_fingerprint


def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv1d(4, 8, 3, padding=1), nn.Sequential(nn.Tanh(), nn.Dropout(0.1)), nn.Conv1d(8, 2, 1))


def _fp(net):
    return model_fingerprint(list(net.parameters()), list(net.modules()))


def test_fingerprint_changes_on_each_kind_of_toggle():
    net = _net()
    base = _fp(net)
    assert base == (tuple([True] * 4), tuple([True] * 6))
    seen = {base}
    for p in net.parameters():                                   # every single parameter, frozen alone
        p.requires_grad_(False)
        fp = _fp(net)
        assert fp not in seen, 'freezing one parameter gives a fingerprint of its own'
        seen.add(fp)
        p.requires_grad_(True)
        assert _fp(net) == base, 'unfreezing it brings the first one back'
    for m in net.modules():                                      # every module's own flag, the container's included
        m.training = False
        fp = _fp(net)
        assert fp not in seen
        seen.add(fp)
        m.training = True
    net[1].eval()                                                # a submodule with children: three flags at once
    assert _fp(net) not in seen
    net.train()
    assert _fp(net) == base


def test_fingerprint_sees_a_change_in_number():
    net = _net()
    base = _fp(net)
    net.add_module('extra', nn.Identity())                       # a module without parameters
    more = _fp(net)
    assert more != base and more[0] == base[0] and len(more[1]) == len(base[1]) + 1
    net.extra = nn.Conv1d(2, 2, 1)
    assert len(_fp(net)[0]) == len(base[0]) + 2
    del net.extra
    assert _fp(net) == base


def test_fingerprint_ignores_values_and_gradients():
    net = _net()
    base = _fp(net)
    assert _fp(net) == base and hash(_fp(net)) == hash(base)     # stable, plain tuples of bools
    with torch.no_grad():
        for p in net.parameters():
            p.add_(1.0)
    net(torch.randn(2, 4, 16)).sum().backward()
    assert all(p.grad is not None for p in net.parameters())
    assert _fp(net) == base
    for p in net.parameters():
        p.grad = None
    assert _fp(net) == base
    net.load_state_dict(_net().state_dict())
    assert _fp(net) == base
    assert _fp(_net()) == base                                   # another instance of the same model in the same state


class _T(Trainer):
    def forward(self, x, y, is_logging=False):
        loss = torch.nn.functional.mse_loss(self.model(x), y)
        return loss, {'loss': (loss.detach(), LogType.SCALAR)}


def _trainer(net, log_interval=10 ** 6):
    g = torch.Generator().manual_seed(1)
    data = [(torch.randn(2, 4, 16, generator=g), torch.randn(2, 2, 16, generator=g)) for _ in range(3)]
    tr = _T(net, torch.optim.SGD(net.parameters(), lr=0.1), data, data[:1], max_step=8, valid_max_step=1, save_interval=10 ** 6,
            log_interval=log_interval, save_dir=tempfile.mkdtemp(prefix='psnd_fp_'), seed=1)
    tr.move_batches_to_gpu = False
    net.train()
    return tr


def test_trainer_drops_its_graphs_when_the_fingerprint_changes():
    """the method around the pure function, with stand-ins for captured steps (no GPU here: a record without a graph is a warm-up
    counter, and that is all reset_graphs looks at before it forgets them)"""
    net = _net()
    tr = _trainer(net)
    tr.train(1)
    assert tr._model_fp == _fp(net)
    tr._graphs = {'sig': CapturedStep(seen=2)}
    tr._opt_cover = ('key', True)
    tr.train(2)                                                  # nothing toggled: graphs, counters and cache stay
    assert tr._graphs == {'sig': CapturedStep(seen=2)} and tr._opt_cover == ('key', True)

    assert all(p.grad is not None for p in net.parameters())
    w = net[0].weight
    w.requires_grad_(False)                                      # its gradient of step 2 is still attached
    kept = w.detach().clone()
    tr.train(3)
    assert tr._graphs == {} and tr._opt_cover is None and tr._model_fp == _fp(net)
    assert w.grad is None and torch.equal(w, kept), 'frozen: no gradient, not stepped'
    assert all(p.grad is not None for p in net.parameters() if p.requires_grad)

    tr._graphs = {'sig': CapturedStep(seen=1)}
    net[1].eval()
    tr.train(4)
    assert tr._graphs == {}
    tr._graphs = {'sig': CapturedStep(seen=1)}
    tr.train(5)
    assert tr._graphs == {'sig': CapturedStep(seen=1)}, 'the same state as at the last step'

    tr.graph_steps = 'auto'
    assert tr._graph_auto_ok is not False, "a toggle does not switch graph_steps = 'auto' off"


def test_reset_graphs_on_request_and_frozen_gradients():
    net = _net()
    tr = _trainer(net)
    net[2].bias.requires_grad_(False)
    net[2].bias.grad = torch.ones_like(net[2].bias)              # left over from before the Trainer saw the model
    tr._graphs = {'sig': CapturedStep(seen=3)}
    tr._opt_cover = ('key', False)
    tr.reset_graphs()
    assert tr._graphs == {} and tr._opt_cover is None
    assert net[2].bias.grad is None
    assert tr._model_fp == _fp(net)
    for i in range(1, 4):
        tr.train(i)
        assert all(p.grad is None for p in net.parameters() if not p.requires_grad)


def test_a_module_added_between_steps_is_seen_on_a_logging_step():
    net = _net()
    tr = _trainer(net, log_interval=2)
    tr.train(1)
    n = len(tr._model_fp[1])
    net.add_module('extra', nn.Identity())
    tr._graphs = {'sig': CapturedStep(seen=1)}
    tr.train(2)                                                  # a logging step: the model is walked again
    assert len(tr._model_fp[1]) == n + 1 and tr._graphs == {}
