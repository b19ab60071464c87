"""Times the YIN pitch tracker of psnd_pitch.hip on a HIP device against its neighbours, same process, same device, alternating.

    python tools/time_f0.py [--blocks 5] [--reps 20] [--out FILE]
    python tools/time_f0.py --one-clip [--reps 20]        # nothing but N = 1 native calls: the run to put under a kernel trace

Shape: 32 clips x 30 s at 22.05 kHz, hop 256, the defaults (71-800 Hz: tau_max = 311, W = 622, threshold 0.1): 2584 frames per clip; and one
such clip.  The clips are three harmonics of a fundamental with vibrato, gated voiced / noise in quarter-second blocks.  Legs per shape:
    native   kernels.yin_f0: one launch, (f0, aperiodicity, lag) on the device
    torch    the same definition in library ops on the device: unfold into frames and into lagged windows, broadcast subtract, square, sum,
             cumsum, comparisons and argmax for the threshold and the descent, gathers for the parabola - in chunks of frames so that the
             (frames, tau_max, W) difference tensor stays under --budget bytes
    host     kernels.yin_f0_host (float64 numpy) on one clip already in host memory, wall time; times 32 for the batch
    copy     what a user without the native path does first: the batch to the host (wall time)

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed calls of its own leg, then times `reps` calls between two
device events (host, copy: a wall clock).  Per leg the median over the blocks and their spread.  For the native legs the arithmetic rate at 3
flops per (j, tau) pair - one subtract, one fused multiply-add - as a fraction of the 157.3 TFLOP/s fp32 vector peak; with one of its two
instructions a plain subtract this mix tops out at 75 % of that figure.
The lags of both device legs are compared with each other at the timed size, and clip 0's native lags with the host restatement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402

SR, HOP, THR = 22050, 256, 0.1
PEAK = 157.3e12


def spin(fn, seconds=0.15):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def device_block(fn, reps):
    spin(fn)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def wall_block(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def summary(ms):
    ms = sorted(ms)
    return {'median_ms': ms[len(ms) // 2], 'min_ms': ms[0], 'max_ms': ms[-1], 'blocks': len(ms)}


def clips(N, T, dev):
    g = torch.Generator(dev).manual_seed(SR)
    t = torch.arange(T, device=dev, dtype=torch.float64) / SR
    base = 90.0 + 220.0 * torch.rand(N, 1, device=dev, generator=g, dtype=torch.float64)
    f = base * (1.0 + 0.03 * torch.sin(2 * np.pi * 5.0 * t + 6.28 * torch.rand(N, 1, device=dev, generator=g, dtype=torch.float64)))
    ph = 2 * np.pi * torch.cumsum(f, dim=1) / SR
    voiced = ((torch.sin(ph) + 0.8 * torch.sin(2 * ph + 0.7) + 0.6 * torch.sin(3 * ph + 1.9)) * (0.9 / 2.4)).float()
    noise = torch.randn(N, T, device=dev, generator=g)
    block = SR // 4
    gate = (torch.rand(N, -(-T // block), device=dev, generator=g) < 0.7).repeat_interleave(block, dim=1)[:, :T]
    return torch.where(gate, voiced + 0.01 * noise, 0.1 * noise)


def torch_f0(x, hop, sr, tau_min, tau_max, W, thr, budget):
    """the definition of include/psnd.h in library ops: (f0, aperiodicity, lag) of an (N, T) float32 tensor"""
    N, T = x.shape
    span = W + tau_max
    F = T // hop + 1
    xp = torch.nn.functional.pad(x, (span // 2, span))
    U = xp.unfold(-1, span, hop)[:, :F]                                 # (N, F, span) view
    taus = torch.arange(1, tau_max + 1, device=x.device)
    in_range = taus >= tau_min
    step = max(1, int(budget // (4 * N * tau_max * W)))
    outs = []
    for a in range(0, F, step):
        u = U[:, a:a + step]
        bad = ~torch.isfinite(u).all(dim=-1)
        e = u[..., None, :W] - u.unfold(-1, W, 1)[..., 1:tau_max + 1, :]
        d = (e * e).sum(dim=-1)                                         # (N, C, tau_max)
        cs = torch.cumsum(d, dim=-1)
        dp = torch.where(cs == 0, torch.ones_like(d), d * taus / cs)
        under = (dp < thr) & in_range
        voiced = under.any(dim=-1) & ~bad
        t0 = under.int().argmax(dim=-1, keepdim=True)
        stop = torch.cat((~(dp[..., 1:] < dp[..., :-1]), torch.ones_like(under[..., :1])), dim=-1) & (taus - 1 >= t0)
        k = stop.int().argmax(dim=-1, keepdim=True)
        y1 = dp.gather(-1, k)
        y0, y2 = dp.gather(-1, (k - 1).clamp(min=0)), dp.gather(-1, (k + 1).clamp(max=tau_max - 1))
        den = y0 - 2.0 * y1 + y2
        ok = (k >= 1) & (k + 1 <= tau_max - 1) & (den > 0)
        off = torch.where(ok, (0.5 * (y0 - y2) / torch.where(ok, den, torch.ones_like(den))).clamp(-0.5, 0.5), torch.zeros_like(den))
        v = voiced[..., None]
        f0 = torch.where(v, sr / (k + 1 + off), torch.zeros_like(off))
        floor = torch.where(in_range, dp, torch.full_like(dp, float('inf'))).amin(dim=-1, keepdim=True)
        ap = torch.where(bad[..., None], torch.ones_like(y1), torch.where(v, y1, floor))
        outs.append((f0[..., 0], ap[..., 0], torch.where(voiced, k[..., 0] + 1, torch.zeros_like(k[..., 0])).int()))
    return tuple(torch.cat([o[i] for o in outs], dim=1) for i in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--budget', type=float, default=2.0 ** 30, help='bytes of the difference tensor of one chunk of the library-op leg')
    ap.add_argument('--one-clip', action='store_true', help='only N = 1 native calls, for a kernel trace')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    N, T = 32, 30 * SR
    tau_min, tau_max, W = K.yin_lags(SR)
    F = K.yin_frames(T, HOP)
    x = clips(N, T, dev)
    one = x[:1].contiguous()
    if a.one_clip:
        for _ in range(a.reps):
            K.yin_f0(one, HOP, SR)
        torch.cuda.synchronize()
        return
    clip0 = x[0].cpu().numpy()
    native = K.yin_f0(x, HOP, SR)
    lib = torch_f0(x, HOP, float(SR), tau_min, tau_max, W, THR, a.budget)
    host = K.yin_f0_host(clip0, HOP, float(SR), tau_min, tau_max, W, THR)
    agree = {'native_vs_torch_lags_equal': float((native[2] == lib[2]).float().mean()),
             'native_vs_host_lags_equal_clip0': float((native[2][0].cpu().numpy() == host[2]).mean()),
             'voiced_fraction': float((native[2] > 0).float().mean())}
    assert agree['native_vs_torch_lags_equal'] > 0.99 and agree['native_vs_host_lags_equal_clip0'] > 0.99, agree
    del lib
    rows = []
    for label, xs, n in (('32 clips', x, N), ('1 clip', one, 1)):
        legs = {
            'native': (device_block, lambda: K.yin_f0(xs, HOP, SR), a.reps),
            'torch': (device_block, lambda: torch_f0(xs, HOP, float(SR), tau_min, tau_max, W, THR, a.budget), 2 if n > 1 else max(a.reps // 4, 2)),
        }
        if n > 1:
            legs['host'] = (wall_block, lambda: K.yin_f0_host(clip0, HOP, float(SR), tau_min, tau_max, W, THR), 1)
            legs['copy'] = (wall_block, lambda: x.cpu(), 2)
        times = {k: [] for k in legs}
        for _ in range(a.blocks):
            for name, (block, fn, reps) in legs.items():
                if name in ('host', 'copy') and len(times[name]) >= 2:
                    continue
                times[name].append(block(fn, reps))
        for name, ms in times.items():
            r = dict(what=name, shape=[1 if name == 'host' else n, T], frames=F, **summary(ms))
            if name == 'host':
                r['scaled_to_32_clips_ms'] = r['median_ms'] * N
            if name == 'native':
                r['flops'] = 3 * n * F * W * tau_max
                r['fraction_of_fp32_vector_peak'] = r['flops'] / (r['median_ms'] * 1e-3) / PEAK
            rows.append(r)
        nat, lib_ms = times['native'], times['torch']
        rows.append(dict(what='native faster than torch in every block', shape=[n, T], value=all(p < q for p, q in zip(nat, lib_ms)),
                         speedup_of_medians=summary(lib_ms)['median_ms'] / summary(nat)['median_ms']))
    for r in rows:
        if 'median_ms' not in r:
            print('%-40s %-14s %s   (medians: %.1f x)' % (r['what'], tuple(r['shape']), r['value'], r['speedup_of_medians']))
            continue
        print('%-7s %-14s median %10.4f ms   min %10.4f   max %10.4f   (%d blocks)%s%s' % (
            r['what'], tuple(r['shape']), r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   %.1f %% of the fp32 vector peak' % (100 * r['fraction_of_fp32_vector_peak']) if 'flops' in r else '',
            '   x 32 = %.1f ms' % r['scaled_to_32_clips_ms'] if 'scaled_to_32_clips_ms' in r else ''))
    print(agree)
    line = json.dumps({'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'agreement': agree, 'rows': rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
