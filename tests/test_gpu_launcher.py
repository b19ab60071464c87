"""_lib.on, the one launch path from Python to the library: the same bits as the call spelled out by hand, the stream that is current at
entry (shown with a hipGraph capture on a side stream), the failure path, and use_library followed by a launcher made before the switch."""
import os

import pytest
import torch

from pytorch_sound_amd import _lib
from pytorch_sound_amd._lib import on, lib, check, ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device('cuda', 0)


@pytest.mark.parametrize('with_res', [True, False])
def test_same_bits_as_the_long_spelling(with_res):
    dev = _dev()
    N, C, T = 2, 4, 70
    g = torch.Generator().manual_seed(3)
    x, r = torch.randn(N, C, T, generator=g).to(dev), torch.randn(N, C, T, generator=g).to(dev)
    res = r if with_res else None                     # None: a NULL pointer argument
    gamma, beta = torch.randn(C, generator=g).to(dev), torch.randn(C, generator=g).to(dev)

    def outputs():
        return (torch.full((N, C, T), 7.0, device=dev), torch.full((N, 2), 7.0, device=dev),
                torch.zeros((N, 2 * C), dtype=torch.float64, device=dev))
    y0, s0, w0 = outputs()
    with torch.cuda.device(dev):
        check(lib().psnd_groupnorm1_fwd(ptr(x), ptr(res), ptr(gamma), ptr(beta), N, C, T, 1e-5, 1, ptr(y0), ptr(s0), ptr(w0), stream_ptr(dev)),
              'psnd_groupnorm1_fwd')
    y1, s1, w1 = outputs()
    with on(dev) as k:
        k.psnd_groupnorm1_fwd(x, res, gamma, beta, N, C, T, 1e-5, 1, y1, s1, w1)
    torch.cuda.synchronize(dev)
    assert torch.equal(y1, y0) and torch.equal(s1, s0)
    assert not (y1 == 7.0).all() and bool(torch.isfinite(y1).all())
    ref = torch.relu(torch.nn.functional.group_norm((x + r if with_res else x).cpu().double(), 1, gamma.cpu().double(), beta.cpu().double(), 1e-5))
    assert (y1.cpu().double() - ref).abs().max() < 1e-4          # (the kernel's own accuracy is another file's subject: this is "it ran")


def test_the_stream_is_the_current_one_at_entry():
    """a launch through on(dev) opened inside a capture on a side stream is captured, not run: the output keeps its sentinel until the replay"""
    dev = _dev()
    N, C, T, scale = 1, 4, 8, 0.5
    x = torch.arange(N * C * T, dtype=torch.float32).reshape(N, C, T).to(dev)
    pe = (torch.arange(C * T, dtype=torch.float32).reshape(C, T) * 0.25).to(dev)
    y = torch.empty_like(x)
    with on(dev) as k:                                # once outside the capture: the kernel's code object is loaded
        k.psnd_posenc(x, pe, scale, N, C, T, T, y)
    y.fill_(-1234.0)
    torch.cuda.synchronize(dev)
    side, graph = torch.cuda.Stream(device=dev), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        with on(dev) as k:
            assert k.stream == side.cuda_stream == torch.cuda.current_stream(dev).cuda_stream
            k.psnd_posenc(x, pe, scale, N, C, T, T, y)
    torch.cuda.synchronize(dev)
    assert bool((y == -1234.0).all()), 'the launch ran during the capture: it went to another stream than the capturing one'
    graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(y, x * scale + pe)


def test_failure_path():
    dev = _dev()
    from pytorch_sound_amd import kernels as K
    n_fft, T = 256, 1000
    plan = K.stft_plan(n_fft, torch.hann_window(n_fft).numpy()).to(dev)
    wav = torch.zeros(1, T, device=dev)
    mag = torch.full((1, n_fft // 2 + 1, K.frame_count(T, n_fft, 64)), 5.0, device=dev)        # what a launch with hop = 64 would write
    with on(dev) as k:
        with pytest.raises(_lib.PsndError) as e:
            k.psnd_stft_fwd(wav, 1, T, n_fft, 0, 0, plan, 0.0, mag, None, None, None)          # hop = 0: rejected on the host
        last = lib().psnd_last_error().decode()
        assert last and 'psnd_stft_fwd' in str(e.value) and last in str(e.value)
        assert '(%d)' % _lib.DEFINES['PSND_E_ARG'] in str(e.value)
        with pytest.raises(TypeError, match='psnd_stft_fwd'):
            k.psnd_stft_fwd(wav, 1, T, n_fft, 64, 0, plan, 0.0, mag, None, None)                # one argument too few
    torch.cuda.synchronize(dev)
    assert bool((mag == 5.0).all())                   # nothing was launched


@pytest.mark.skipif(not os.path.exists(_lib.LAB_LIB_PATH), reason='the lab library (python -m pytorch_sound_amd._build --lab) is not built')
def test_use_library_is_followed(monkeypatch):
    dev = _dev()
    calls = []
    with on(dev) as k:                                # made before the switch
        stream = k.stream
        with _lib.use_library(_lib.LAB_LIB_PATH) as lab:
            assert lab is not None and lab is lib()

            def stub(*args):
                calls.append(args)
                return 0
            monkeypatch.setattr(lab, 'psnd_posenc', stub)
            k.psnd_posenc(None, None, 1.0, 0, 0, 0, 0, None)
        assert calls == [(None, None, 1.0, 0, 0, 0, 0, None, stream)]
        assert lib() is not lab
