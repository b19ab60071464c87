"""LearnableSTFT's native entry points (psnd_lstft_*) as far as a machine without a GPU can check them: exported and bound, the slab
count of the basis gradient, argument validation before any device work, and the untouched CPU path of the module through the public
alias package."""
import ctypes
import os

import numpy as np
import pytest
import torch

NAMES = ('psnd_lstft_analysis', 'psnd_lstft_mag_bwd', 'psnd_lstft_synthesis', 'psnd_lstft_wgrad_slabs', 'psnd_lstft_basis_grad')
E_ARG = -1


@pytest.fixture(scope='module')
def L():
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    return _lib


def _buf():
    buf = (ctypes.c_float * 8)()
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def test_entry_points_exported_and_bound(L):
    h = ctypes.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert hasattr(h, n), 'the library does not export %s' % n
        assert n in L.SIGNATURES, '%s is missing from the ctypes table' % n
        assert getattr(L.lib(), n).argtypes == L.SIGNATURES[n][1]
    assert L.lib().psnd_version() >= 138


def test_wgrad_slabs_positive_and_deterministic(L):
    lib = L.lib()
    for N, C, n, F in [(32, 1026, 1024, 126), (32, 258, 256, 501), (1, 258, 256, 1), (3, 152, 150, 55), (8, 1026, 1024, 1025), (1, 2, 2, 1)]:
        s = lib.psnd_lstft_wgrad_slabs(N, C, n, F)
        assert s > 0 and s == lib.psnd_lstft_wgrad_slabs(N, C, n, F)
        assert s <= 4096                                             # a workspace of a few slabs per compute unit, not one per frame
    assert lib.psnd_lstft_wgrad_slabs(0, 258, 256, 10) == 0


def _err(L):
    msg = L.lib().psnd_last_error()
    assert msg, 'no message in psnd_last_error'
    return msg.decode()


def test_argument_validation_without_gpu(L):
    lib = L.lib()
    keep, p = _buf()
    ok = dict(N=2, Lx=1000, C=258, n=256, hop=64)

    def analysis(x=p, b=p, w=p, spec=p, mag=None, phase=None, **kw):
        a = dict(ok, **kw)
        return lib.psnd_lstft_analysis(x, b, w, a['N'], a['Lx'], a['C'], a['n'], a['hop'], spec, mag, phase, None)

    def synthesis(g=p, b=p, w=p, y=p, F=10, Ly=None, **kw):
        a = dict(ok, **kw)
        Ly = a['n'] + a['hop'] * (F - 1) if Ly is None else Ly
        return lib.psnd_lstft_synthesis(g, b, w, None, a['N'], a['C'], F, a['n'], a['hop'], Ly, y, None)

    def grad(g=p, x=p, w=p, part=p, gb=p, F=10, **kw):
        a = dict(ok, **kw)
        return lib.psnd_lstft_basis_grad(g, x, w, a['N'], a['Lx'], a['C'], a['n'], a['hop'], F, part, gb, None)

    for call in (analysis, synthesis, grad):
        for bad in (dict(hop=0), dict(hop=-3)):
            assert call(**bad) == E_ARG and 'hop' in _err(L)
        assert call(n=1) == E_ARG and 'n=1' in _err(L)
    assert analysis(Lx=255) == E_ARG and 'shorter' in _err(L)
    assert grad(Lx=255) == E_ARG and 'shorter' in _err(L)
    assert synthesis(Ly=255, F=1) == E_ARG and 'shorter' in _err(L)
    assert synthesis(F=10, Ly=256 + 64 * 9 - 1) == E_ARG and 'frames' in _err(L)          # rows of y shorter than the frames reach
    assert grad(F=13) == E_ARG and 'frames' in _err(L)                                     # (1000 - 256) // 64 + 1 = 12 frames at most
    assert analysis(C=257, mag=p, phase=p) == E_ARG and 'pair' in _err(L)                  # odd C with mag / phase requested
    assert analysis(C=258, mag=p) == E_ARG                                                 # mag without phase
    for null in ('x', 'b', 'w', 'spec'):
        assert analysis(**{null: None}) == E_ARG and 'null' in _err(L)
    for null in ('g', 'b', 'w', 'y'):
        assert synthesis(**{null: None}) == E_ARG and 'null' in _err(L)
    for null in ('g', 'x', 'w', 'part', 'gb'):
        assert grad(**{null: None}) == E_ARG and 'null' in _err(L)
    assert lib.psnd_lstft_mag_bwd(p, p, None, 1, 258, 4, p, None) == E_ARG and 'null' in _err(L)
    assert lib.psnd_lstft_mag_bwd(p, p, p, 1, 257, 4, p, None) == E_ARG
    del keep


def test_cpu_path_unchanged_through_public_alias():
    """the golden of tests/test_filters_golden.py once more, through `pytorch_sound.models.transforms` (CPU tensors: the reference's
    own convolutions, whether or not the native library is there)"""
    from pytorch_sound.models.transforms import LearnableSTFT
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'lstft.npz'))
    m = LearnableSTFT(256, 64, 200)
    assert sorted(m.state_dict().keys()) == list(g['state_keys'])
    mag, phase = m.transform(torch.from_numpy(g['wav']))
    rec = m.inverse(mag, phase)
    (mag.sum() + rec.pow(2).sum()).backward()
    assert not phase.requires_grad
    assert np.abs(mag.detach().numpy() - g['mag']).max() < 2e-5 * np.abs(g['mag']).max()
    assert np.abs(rec.detach().numpy() - g['rec']).max() < 1e-4 * np.abs(g['rec']).max()
    rows = [0, 1, 64, 129, 200, 257]
    for grad, want in ((m.forward_basis.grad, g['g_forward_basis_rows']), (m.inverse_basis.grad, g['g_inverse_basis_rows'])):
        assert np.abs(grad.numpy()[rows] - want).max() < 1e-3 * max(np.abs(want).max(), 1e-6)
