"""Dropout, the parts that need no GPU: the numpy Philox4x32-10 that tests/test_gpu_dropout.py recomputes the kernels' masks with gives the
published known answers, the host-side threshold / scale are the specified ones, the new entry points reject bad arguments before they touch
a device, and CPU tensors keep nn.Dropout."""
import ctypes

import numpy as np
import pytest
import torch

import test_gpu_dropout as G


@pytest.fixture(autouse=True)
def _global_generator_untouched():
    """module initialisation and nn.Dropout draw from torch's process-wide CPU generator: it is handed back as it was found"""
    cpu = torch.get_rng_state()
    yield
    torch.set_rng_state(cpu)


def test_numpy_philox_known_answers():
    G.test_numpy_philox_known_answers()


def test_keep_mask_indexing():
    """element i takes word i % 4 of quad i // 4, whatever the shape: a (3, 8, 50) tensor's rows start inside a quad"""
    flat = G.keep_mask((1200,), 5, 9, 0.5)
    assert np.array_equal(G.keep_mask((3, 8, 50), 5, 9, 0.5).reshape(-1), flat)
    words = G.philox4x32_10(np.array([[299, 0, 9, 0]], dtype=np.uint64), (5, 0))[0]
    assert list(flat[1196:1200]) == [bool(w >= (1 << 31)) for w in words]
    assert not np.array_equal(flat, G.keep_mask((1200,), 5, 10, 0.5)) and not np.array_equal(flat, G.keep_mask((1200,), 6, 9, 0.5))
    assert not np.array_equal(flat, G.keep_mask((1200,), 5 + (1 << 32), 9, 0.5)) and not np.array_equal(flat, G.keep_mask((1200,), 5, 9 + (1 << 32), 0.5))


def test_threshold_and_scale():
    from pytorch_sound_amd import kernels as K
    for p in (0.1, 0.5, 0.25, 1e-12, 1.0 - 2.0 ** -24):
        assert K.dropout_threshold(p) == (G.drop_thr(p), G.drop_scale(p))
    assert K.dropout_threshold(0.5) == (1 << 31, 2.0)
    assert K.dropout_threshold(0.1)[1] == float(np.float32(1.0) / np.float32(0.9))
    for p in (0.0, 1.0, -0.1, 1.5, 1.0 - 2.0 ** -40):       # (the last one is 1 in fp32: no finite scale)
        with pytest.raises(K.PsndError):
            K.dropout_threshold(p)


def test_entry_points_reject_bad_arguments():
    from pytorch_sound_amd import _build, _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.psnd_rng_seed(None, 1, 0, None) == -1 and lib.psnd_rng_next(None, p, None) == -1 and lib.psnd_rng_next(p, p, None) == -1
    assert lib.psnd_groupnorm1_drop_fwd(p, p, p, p, 1, 4, 4, 1e-5, 0, p, p, p, None, 1 << 31, 2.0, None) == -1       # no key
    assert lib.psnd_groupnorm1_drop_fwd(p, p, p, p, 1, 4, 4, 1e-5, 0, p, p, p, p, 1 << 31, 0.5, None) == -1          # scale below 1
    assert lib.psnd_groupnorm1_drop_fwd(p, p, p, p, 0, 4, 4, 1e-5, 0, p, p, p, p, 1 << 31, 2.0, None) == 0           # empty batch
    assert lib.psnd_groupnorm1_drop_fwd(p, p, p, p, 1, 0, 4, 1e-5, 0, p, p, p, p, 1 << 31, 2.0, None) == -2
    assert lib.psnd_groupnorm1_drop_bwd(p, p, p, p, p, p, 1, 4, 4, 0, p, p, p, p, p, p, 1 << 31, 2.0, None) == -1    # gres aliases gx
    assert lib.psnd_groupnorm1_drop_bwd(p, p, None, p, p, p, 1, 4, 4, 0, p, None, p, p, p, None, 1 << 31, 2.0, None) == -1
    assert lib.psnd_groupnorm1_drop_bwd(p, p, None, p, p, p, 0, 4, 4, 0, p, None, p, p, p, p, 1 << 31, 2.0, None) == 0


def test_cpu_tensors_keep_nn_dropout():
    from pytorch_sound_amd.models.modules import MultiHeadAttention, PointwiseFeedForward
    for rate in (0.0, 1.0):
        assert MultiHeadAttention(16, 4, rate).drop_out is None and PointwiseFeedForward(16, rate).drop_out is None
    mha, ffn = MultiHeadAttention(16, 4, 0.5).train(), PointwiseFeedForward(16, 0.5).train()
    x = torch.from_numpy(np.random.RandomState(0).randn(2, 16, 10).astype(np.float32))
    calls = []
    for m in (mha, ffn):
        m.drop_out.register_forward_hook(lambda mod, a, out: calls.append(mod.training))
    y = ffn(mha(x)[0])
    assert calls == [True, True] and y.shape == x.shape
    assert not torch.equal(ffn(x), ffn(x)), 'training mode drops'
    ffn.eval()
    assert torch.equal(ffn(x), ffn(x))
