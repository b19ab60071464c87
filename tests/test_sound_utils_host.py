"""Host-side rules of the native VolNormConv / InversePreEmphasis paths (models/sound.py): the slice layout the launch is sized by, against a
brute-force run of the class's own python loops, and the warm-up rule of the time-parallel scan against its error bound."""
import pytest
import torch

from pytorch_sound_amd import kernels as K
from pytorch_sound_amd.models.sound import VolNormConv, ipreemph_warm, volnorm_layout


def _run_class(L, window, hop, reverse):
    """(hops, output length) of the class's own loop on a CPU signal: every hop asks _scale once"""
    vn = VolNormConv(window, hop, 0.0)
    calls = []
    vn._scale = lambda std: calls.append(1) or 1.0
    x = torch.zeros(2, L)
    if reverse:
        vn.init_buffer(L)
    out = vn.reverse(x) if reverse else vn.forward(x)
    return len(calls), out.size(-1)


def _brute(L, window, hop, reverse):
    """(start, samples) of every slice, by the slicing lines of forward / reverse on a ramp"""
    last = L - window
    pieces = []
    for start in range(0, last, hop):
        if reverse:
            stop = start + hop if start < last - hop else None
        else:
            stop = start + hop if start < last - 1 else None
        pieces.append((start, torch.arange(L)[start:stop]))
    return pieces


def _triples():
    out = []
    for window in (1, 3, 8, 400):
        for hop in (1, 2, 5, 7, 160, 401, 403, 1000):
            for extra in (1, 2, 3, hop - 1, hop, hop + 1, 2 * hop, 2 * hop + 1, 3 * hop - 1, 5 * hop + 2):
                if extra >= 1:
                    out.append((window + extra, window, hop))
    return sorted(set(out))


TRIPLES = _triples()


def test_triples_cover_the_edge_cases():
    assert len(TRIPLES) >= 200
    last_hop = lambda L, w, h: (volnorm_layout(L, w, h)[0] - 1) * h                      # noqa: E731
    assert any((L - w) % h == 0 and (L - w) // h >= 2 for L, w, h in TRIPLES)
    assert any(last_hop(L, w, h) == L - w - 1 and last_hop(L, w, h) > 0 for L, w, h in TRIPLES)      # a tail that runs to the end
    assert any(h > w + 2 and L - w > h for L, w, h in TRIPLES)                           # a clamped or dropped tail
    assert any(L == w + 1 for L, w, h in TRIPLES)


@pytest.mark.parametrize('reverse', [False, True])
def test_volnorm_layout_matches_the_loops(reverse):
    for L, window, hop in TRIPLES:
        pieces = _brute(L, window, hop, reverse)
        n_hops, out_len, tail_start = volnorm_layout(L, window, hop, reverse)
        assert n_hops == len(pieces) >= 1, (L, window, hop)
        assert (n_hops, out_len) == _run_class(L, window, hop, reverse), (L, window, hop)
        assert out_len == sum(len(p) for _, p in pieces), (L, window, hop)
        assert n_hops <= (L - window) // hop + 1                                         # std_buffer holds them
        pos = 0
        for i, (start, p) in enumerate(pieces):                                          # hop i fills [i * hop, ...) of the output
            assert start == i * hop == pos and len(p) >= 1, (L, window, hop)
            if start >= tail_start:
                assert i == n_hops - 1 and int(p[-1]) == L - 1, (L, window, hop)
            else:
                assert len(p) == min(hop, L - start), (L, window, hop)
            pos += len(p)
        if reverse:
            assert out_len == L


def test_volnorm_layout_without_a_hop():
    for L, window, hop in ((400, 400, 160), (10, 400, 160), (0, 1, 1)):
        assert volnorm_layout(L, window, hop)[:2] == (0, 0) and volnorm_layout(L, window, hop, True)[:2] == (0, 0)


def test_warm_up_rule():
    for c in (0.5, 0.9, 0.97, -0.97, 0.99, 1e-3, 0.0, 1e-30):
        W = ipreemph_warm(c)
        assert 32 <= W <= K.IPREEMPH_WARM_MAX and W % 32 == 0, (c, W)
        assert 2.0 * abs(c) ** W <= 2.0 ** -25, (c, W)
        assert W == 32 or 2.0 * abs(c) ** (W - 32) > 2.0 ** -25, (c, W)                  # and no longer than the rule asks
    assert ipreemph_warm(0.97) == 608                                                    # 592 steps, to the next multiple of 32
    for c in (1.0, -1.0, 1.5, 0.9999, 0.995, float('nan'), float('inf')):
        assert ipreemph_warm(c) == K.IPREEMPH_SEQ, c
    # the seam between the instances is where the warm-up stops fitting the kernel's LDS image
    assert ipreemph_warm(0.9912) > 0 and ipreemph_warm(0.9913) == K.IPREEMPH_SEQ


def test_entry_points_validate_before_touching_the_device():
    import ctypes
    import os
    from pytorch_sound_amd import _build, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _build.build(verbose=False)
    lib = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.psnd_ipreemph_fwd(None, 1, 8, p, p, K.IPREEMPH_AUTO, p, None) == -1
    assert lib.psnd_ipreemph_fwd(p, 1, 8, p, None, K.IPREEMPH_AUTO, p, None) == -1                 # the weights are pointers too
    assert lib.psnd_ipreemph_fwd(p, 1, 8, p, p, 33, p, None) == -1                                 # warm-up: a multiple of 32 ...
    assert lib.psnd_ipreemph_fwd(p, 1, 8, p, p, K.IPREEMPH_WARM_MAX + 32, p, None) == -1           # ... that fits the LDS image
    assert lib.psnd_ipreemph_fwd(p, 70000, 8, p, p, 608, p, None) == -2
    assert lib.psnd_ipreemph_fwd(p, 0, 8, p, p, 608, p, None) == 0 and lib.psnd_ipreemph_fwd(p, 3, 0, p, p, K.IPREEMPH_SEQ, p, None) == 0
    assert lib.psnd_ipreemph_bwd(p, p, p, 1, 8, p, p, -3, p, p, p, None) == -1
    assert lib.psnd_ipreemph_bwd(p, p, p, 1, 8, p, p, 608, p, None, p, None) == -1                 # no scratch for the partial sums
    n_hops, out_len, _ = volnorm_layout(4000, 400, 160)
    assert lib.psnd_volnorm_fwd(None, 1, 4000, 400, 160, 1.0, p, out_len, p, None) == -1
    assert lib.psnd_volnorm_fwd(p, 1, 400, 400, 160, 1.0, p, 400, p, None) == -2                   # no hop
    assert lib.psnd_volnorm_fwd(p, 1, 4000, 400, 160, 1.0, p, 4001, p, None) == -2                 # output longer than the signal
    assert lib.psnd_volnorm_fwd(p, 1, 4000, 400, 160, 1.0, p, (n_hops - 1) * 160, p, None) == -2   # the last hop's slice would be empty
    assert lib.psnd_volnorm_reverse(p, 1, 4000, 400, 0, 1.0, p, p, 4000, None) == -1
    assert lib.psnd_volnorm_reverse(p, 0, 4000, 400, 160, 1.0, p, p, 4000, None) == -2
    assert b'volnorm_reverse' in lib.psnd_last_error()
