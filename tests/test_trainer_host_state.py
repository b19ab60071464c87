"""Trainer.graph_steps = 'auto' decides whether a forward() may be captured by watching the host-side state it could draw from.  A draw the
fingerprint misses is a captured step that replays the first decision forever - these pin that every kind of draw changes it, from a warm
state (numpy's position counter inside the key block, a cached gaussian), and that nothing else does."""
import random

import numpy as np
import pytest
import torch

from pytorch_sound_amd.trainer import _GeneratorWatch, _host_rng_fingerprint

DRAWS = {
    'numpy_rand': lambda: np.random.rand(),
    'numpy_randint': lambda: np.random.randint(1000),
    'numpy_second_randn': lambda: np.random.randn(),           # after the warm randn: served from the gauss cache, the key does not move
    'python_random': lambda: random.random(),
    'torch_rand': lambda: torch.rand(()),
}


def _warm(kind):
    random.seed(11)
    np.random.seed(11)
    torch.manual_seed(11)
    if kind == 'numpy_second_randn':
        np.random.randn()                                       # draws a pair, hands out one, caches the other
        assert np.random.get_state()[3] == 1
    else:
        np.random.rand()
    random.random()
    torch.rand(())
    assert np.random.get_state()[2] < 624                       # not at a block boundary: the next draw does not refill the key


@pytest.mark.parametrize('kind', sorted(DRAWS))
def test_fingerprint_changes_after_each_kind_of_draw(kind):
    _warm(kind)
    before = _host_rng_fingerprint()
    key = np.random.get_state()[1].copy()
    DRAWS[kind]()
    assert _host_rng_fingerprint() != before
    assert np.array_equal(np.random.get_state()[1], key)        # (the case the key-only hash missed)


def test_fingerprint_is_stable_without_a_draw():
    _warm('numpy_rand')
    before = _host_rng_fingerprint()
    x = torch.ones(3) * 2 + np.float32(1.0)                     # tensor / numpy arithmetic, no generator
    rs = np.random.RandomState(0)
    rs.rand()                                                   # a generator object of its own: not the global state (and not observable)
    assert float(x.sum()) == 9.0
    assert _host_rng_fingerprint() == before
    assert _host_rng_fingerprint() == _host_rng_fingerprint()


def test_generator_watch_sees_explicit_generators_only():
    g = torch.Generator().manual_seed(3)
    with _GeneratorWatch() as w:
        torch.randn(4).sum()
        torch.ones(2, 2).matmul(torch.ones(2, 2))
    assert not w.used                                           # the default generator is the fingerprint's business
    with _GeneratorWatch() as w:
        torch.rand((), generator=g)
    assert w.used
    with _GeneratorWatch() as w:
        torch.empty(5).uniform_(0, 1, generator=g)
    assert w.used
    with _GeneratorWatch() as w:
        torch.randperm(6, generator=g)
    assert w.used
