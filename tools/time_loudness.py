"""Times the loudness meter of psnd_loudness.hip on a HIP device against its neighbours, same process, same device, alternating.

    python tools/time_loudness.py [--blocks 7] [--reps 20] [--out FILE]
    python tools/time_loudness.py --one-clip [--reps 20]        # nothing but N = 1 native calls: the run to put under a kernel trace
    python tools/time_loudness.py --count-launches              # kernels per call of the native and the composed path (torch.profiler)

Shapes: 32 clips x 30 s at 44.1 kHz, and one clip; noise whose level steps every quarter second, four stretches in ten 50 dB down.  Legs:
    native       kernels.loudness: at most three launches, every sample read once per launch, LUFS on the device
    native N=1   the same on one clip
    composed     the same definition from what the project had before: kernels.lfilter twice (the shelf, then the high-pass: two full-size
                 fp32 intermediates written and read back, four launches), then square / unfold / mean / the two masked means in library
                 ops in float64
    normalize    utils.sound.normalize(kind='ebu'): the meter, then psnd_gain_rows
    level        kernels.level('rms'): psnd_row_level, one workgroup per clip
    host         kernels.loudness_host (float64 numpy, scipy's lfilter) on one clip already in host memory, wall time, times 32
    copy         what a user without the native path does first: the batch to the host (wall time)

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed calls of its own leg, then times `reps` calls between two
device events (host, copy: a wall clock).  Per leg the median over the blocks and their spread; for the native legs the bytes of the floor
(4 B per sample: the input read once) over time as a fraction of 8 TB/s.  The meter reads the input twice (the carry launch and the energy
launch) and writes next to nothing, so the floor fraction is at most one half of what the memory system delivers to it.
The native LUFS of every clip are compared with the composed path and, for clip 0, with the host restatement at the timed size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402
from pytorch_sound_amd.utils import sound as U                                       # noqa: E402

SR = 44100


def spin(fn, seconds=0.15):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(10):
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
    block = SR // 4
    quiet = (torch.rand(N, -(-T // block), device=dev, generator=g) < 0.4).repeat_interleave(block, dim=1)[:, :T]
    noise = torch.randn(N, T, device=dev, generator=g)
    return torch.where(quiet, 3e-4 * noise, 0.1 * noise)


def composed(x, sr):
    """the definition from kernels.lfilter and library ops: LUFS per row (the intermediates are fp32, the block sums float64)"""
    (b1, a1), (b2, a2) = K.k_weighting(sr)
    B, H = K.loudness_block(sr)
    y = K.lfilter(K.lfilter(x, b1, a1), b2, a2)
    z = (y.double() ** 2).unfold(-1, B, H).mean(dim=-1)
    above = z > K.LOUDNESS_GATE
    gamma = 0.1 * (z * above).sum(dim=-1) / above.sum(dim=-1)
    keep = above & (z > gamma[:, None])
    return (-0.691 + 10.0 * torch.log10((z * keep).sum(dim=-1) / keep.sum(dim=-1))).float()


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'Memcpy' not in e.name and 'Memset' not in e.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--one-clip', action='store_true', help='only N = 1 native calls, for a kernel trace')
    ap.add_argument('--count-launches', action='store_true', help='count the kernels of one call of each device leg and stop')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    N, T = 32, 30 * SR
    x = clips(N, T, dev)
    one = x[:1]
    if a.one_clip:
        for _ in range(a.reps):
            K.loudness(one, SR)
        torch.cuda.synchronize()
        return
    device_legs = {
        'native': (lambda: K.loudness(x, SR), N),
        'native N=1': (lambda: K.loudness(one, SR), 1),
        'composed': (lambda: composed(x, SR), N),
        'composed N=1': (lambda: composed(one, SR), 1),
        'normalize': (lambda: U.normalize(x, SR, -23.0), N),
        'level': (lambda: K.level(x, 'rms'), N),
    }
    if a.count_launches:
        print(json.dumps({'kernels_per_call': {k: count_kernels(fn) for k, (fn, _) in device_legs.items()}}))
        return
    clip0 = x[0].cpu().numpy()
    native, comp, host = K.loudness(x, SR), composed(x, SR), float(K.loudness_host(clip0, SR))
    worst = float((native - comp).abs().max())
    assert bool(torch.isfinite(native).all()) and worst < 1e-3 and abs(float(native[0]) - host) < 1e-4, (worst, float(native[0]), host)
    legs = {k: (device_block, fn, a.reps if 'composed' not in k else max(a.reps // 4, 2), n) for k, (fn, n) in device_legs.items()}
    legs['host'] = (wall_block, lambda: K.loudness_host(clip0, SR), 2, 1)
    legs['copy'] = (wall_block, lambda: x.cpu(), 2, N)
    times = {k: [] for k in legs}
    for _ in range(a.blocks):
        for name, (block, fn, reps, _) in legs.items():
            if name in ('host', 'copy') and len(times[name]) >= 3:
                continue
            times[name].append(block(fn, reps))
    rows = []
    for name, ms in times.items():
        n = legs[name][3]
        r = dict(what=name, shape=[n, T], sr=SR, **summary(ms))
        if name == 'host':
            r['scaled_to_32_clips_ms'] = r['median_ms'] * N
        if name not in ('host', 'copy'):
            r['floor_bytes'] = 4 * n * T
            r['floor_fraction_of_8TBps'] = r['floor_bytes'] / (r['median_ms'] * 1e-3) / 8e12
        rows.append(r)
    for r in rows:
        print('%-13s %-14s median %10.4f ms   min %10.4f   max %10.4f   (%d blocks)%s%s' % (
            r['what'], tuple(r['shape']), r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   floor %.2f %% of 8 TB/s' % (100 * r['floor_fraction_of_8TBps']) if 'floor_bytes' in r else '',
            '   x 32 = %.1f ms' % r['scaled_to_32_clips_ms'] if 'scaled_to_32_clips_ms' in r else ''))
    line = json.dumps({'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'native_minus_composed_max_lu': worst,
                       'native_clip0_lufs': float(native[0]), 'host_clip0_lufs': host, 'rows': rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
