#!/usr/bin/env python
"""Mixed-radix STFT kernels (psnd_stft_mr_*) against the dense-basis path of `STFT` (dense.py) at speech framings: 32 clips x 2 s at
(400, 160) / 16 kHz, (1200, 300) / 24 kHz, (2400, 600) / 48 kHz.  Per direction: mean of 64 launches behind at least 150 ms of untimed
launches; algorithmic bytes (4NT + 4NKF per output tensor) over time as a fraction of 8 TB/s.

    python tools/time_stft_mr.py [--json FILE]
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pytorch_sound_amd.models.transforms import STFT, STFTTorchAudio  # noqa: E402

DEV = torch.device('cuda:0')
SHAPES = [(400, 160, 16000), (1200, 300, 24000), (2400, 600, 48000)]
N, SECONDS, REPS, WARM_S = 32, 2, 64, 0.15


def timed(fn):
    """mean seconds of REPS launches of fn, events on the launch stream, after >= WARM_S of untimed launches"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < WARM_S:
        for _ in range(8):
            fn()
        torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3 / REPS


def directions(mod, wav, magnitude):
    """(forward, backward, inverse) closures of one module; the backward is the gmag adjoint alone (the graph is built once)"""
    x = wav.clone().requires_grad_(True)
    mag = magnitude(mod, x)
    g = torch.randn_like(mag)
    with torch.no_grad():
        m0, p0 = mod.transform(wav)
        m0, p0 = m0.contiguous(), p0.contiguous()
    return (lambda: magnitude(mod, wav),
            lambda: torch.autograd.grad(mag, x, g, retain_graph=True),
            lambda: mod.inverse(m0, p0))


def main():
    rows = []
    for n, hop, sr in SHAPES:
        T = SECONDS * sr
        wav = torch.randn(N, T, device=DEV) * 0.07
        K, F = n // 2 + 1, T // hop + 1
        byt = 4 * N * T + 4 * N * K * F
        new = STFTTorchAudio(n, hop).to(DEV)
        old = STFT(n, hop).to(DEV)
        t_new, t_old = [None] * 3, [None] * 3
        fn_new = directions(new, wav, lambda m, w: m.transform(w)[0])
        fn_old = directions(old, wav, lambda m, w: m.magnitude(w))
        for i in range(3):
            if i != 1:
                with torch.no_grad():
                    t_new[i], t_old[i] = timed(fn_new[i]), timed(fn_old[i])
            else:
                t_new[i], t_old[i] = timed(fn_new[i]), timed(fn_old[i])
        for name, a, b in zip(('magnitude forward', 'gmag backward', 'inverse'), t_new, t_old):
            rows.append(dict(n_fft=n, hop=hop, sample_rate=sr, N=N, T=T, direction=name, mixed_radix_us=a * 1e6, dense_us=b * 1e6,
                             bytes=byt, mixed_radix_frac_8TBs=byt / a / 8e12, dense_frac_8TBs=byt / b / 8e12))
            print('n=%d hop=%d %-18s mixed-radix %8.1f us (%.1f%% of 8 TB/s)   dense %8.1f us (%.1f%%)   x%.2f'
                  % (n, hop, name, a * 1e6, 100 * byt / a / 8e12, b * 1e6, 100 * byt / b / 8e12, b / a), flush=True)
        del wav, fn_new, fn_old
    if '--json' in sys.argv:
        with open(sys.argv[sys.argv.index('--json') + 1], 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
