#!/usr/bin/env python
"""LearnableSTFT training step: transform + inverse + backward (both bases trainable, waveform gradient wanted) at 32 clips of 2 s @ 16 kHz,
filter / hop 1024 / 256 and 256 / 64.  Only the module's public API is used, so the same file times any checkout of the package
(PYTHONPATH, or run it from that checkout's tools/): a revision that takes the library convolutions against one on psnd_lstft_*.
Mean of 64 steps behind >= 150 ms of untimed ones; the analysis product's share of the 157 TF fp32-matrix peak is printed for scale
(2 * 2K * n flop per frame; a step runs the equivalent of six such products)."""
import os
import sys
import time
import torch

sys.path.insert(0, os.environ.get('PSND_TREE', os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from pytorch_sound_amd.models.transforms import LearnableSTFT  # noqa: E402

dev = torch.device('cuda:0')


def timeit(f, n=64, warm_ms=150.0):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < warm_ms:
        f()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


for n, hop in ((1024, 256), (256, 64)):
    torch.manual_seed(0)
    m = LearnableSTFT(n, hop).to(dev)
    wav = (0.1 * torch.randn(32, 32000, device=dev)).requires_grad_(True)

    def step():
        wav.grad = None
        for p in m.parameters():
            p.grad = None
        mag, phase = m.transform(wav)
        rec = m.inverse(mag, phase)
        (mag.sum() + rec.pow(2).sum()).backward()

    def fwd():
        with torch.no_grad():
            m.transform(wav)

    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    print('LearnableSTFT(%d, %d): first step (library load, and a convolution library\'s kernel search where one is used) %.1f s'
          % (n, hop, time.perf_counter() - t0), flush=True)
    t_step, t_fwd = timeit(step), timeit(fwd)
    frames = 32 * (32000 // hop + 1)
    flop = 2.0 * m.forward_basis.shape[0] * n * frames
    print('LearnableSTFT(%d, %d) 32 x 32000: transform + inverse + backward %.3f ms; transform alone %.3f ms (%.2f GF: at most %.1f %% of the '
          '157 TF fp32-matrix peak, padding and polar pass included)' % (n, hop, t_step, t_fwd, flop / 1e9, 100 * flop / (t_fwd * 1e-3) / 157e12),
          flush=True)
