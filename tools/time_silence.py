"""Times the silence detector of psnd_silence.hip on a HIP device against its neighbours, same process, same device, alternating.

    python tools/time_silence.py [--blocks 7] [--reps 20] [--out FILE]
    python tools/time_silence.py --one-clip [--reps 20]        # nothing but N = 1 calls: the run to put under a kernel trace

Shape: 32 clips x 30 s at 44.1 kHz, gated noise (quarter-second blocks, four in ten quiet).  Two parameter sets: (1000 samples, -40 dB, step 1)
- a start at every sample - and the preprocess script's (5000, -50 dB, step sr / 2).  Legs per set:
    native       kernels.silence_ranges: three launches, count and ranges on the device
    native N=1   the same on one clip: the range kernel is one workgroup per row, this is where it shows
    torch        the DECISIONS only (no merging into ranges) by the same definition in library ops: float64 cumsum of x^2 over the row and two
                 gathers per start.  This is the row-long prefix the kernels avoid: it is inexact behind loud passages and is
                 here for its cost alone
    host         the numpy restatement (kernels.silence_ranges_host) on one clip already in host memory, wall time, times 32
    copy         what a user without the native path does first: the batch to the host (wall time)

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed calls of its own leg, then times `reps` calls between two
device events (host, copy: a wall clock).  Per leg the median over the blocks and their spread; for the native legs bytes over time as a
fraction of 8 TB/s, twice: for the floor (4 B per sample: the input read once) and for what this design moves at step 1 (A reads 4 B and
writes 12 B of prefixes per sample, B reads them back once - neighbouring starts share them - and a flag byte per start is written and read:
28 B per sample and 2 B per start; at a wide step B reads less, the figure is then an upper bound).
The native ranges of clip 0 are compared with the host restatement at the timed size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402

SR = 44100
SETS = (('every sample', 1000, -40.0, 1), ('preprocess', 5000, -50.0, SR // 2))


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
    return torch.where(quiet, 1e-4 * noise, 0.1 * noise)


def torch_decisions(x, L, s, theta):
    """the definition's decisions from one row-long float64 prefix sum (inexact: module docstring)"""
    T = x.shape[-1]
    P = torch.nn.functional.pad(torch.cumsum(x.double() ** 2, dim=-1), (1, 0))
    i = torch.arange(0, T - L + 1, s, device=x.device)
    if (T - L) % s:
        i = torch.cat((i, i.new_tensor([T - L])))
    return (P[:, i + L] - P[:, i]) <= theta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--one-clip', action='store_true', help='only N = 1 native calls of both parameter sets, for a kernel trace')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    N, T = 32, 30 * SR
    x = clips(N, T, dev)
    one = x[:1]
    if a.one_clip:
        for _, L, db, s in SETS:
            for _ in range(a.reps):
                K.silence_ranges(one, L, db, s)
        torch.cuda.synchronize()
        return
    clip0 = x[0].cpu().numpy()
    rows = []
    for label, L, db, s in SETS:
        theta = K.silence_theta(L, db)
        S = int(K.lib().psnd_silence_starts(T, L, s))
        count, ranges = K.silence_ranges(x, L, db, s)
        want = K.silence_ranges_host(clip0, L, s, theta)
        assert int(count[0]) == len(want) > 0 and np.array_equal(ranges[0, :len(want)].cpu().numpy(), want), label
        legs = {
            'native': (device_block, lambda: K.silence_ranges(x, L, db, s), a.reps, N),
            'native N=1': (device_block, lambda: K.silence_ranges(one, L, db, s), a.reps, 1),
            'torch': (device_block, lambda: torch_decisions(x, L, s, theta), max(a.reps // 4, 2), 0),
            'host': (wall_block, lambda: K.silence_ranges_host(clip0, L, s, theta), 1 if s == 1 else 20, 0),
            'copy': (wall_block, lambda: x.cpu(), 2, 0),
        }
        times = {k: [] for k in legs}
        for _ in range(a.blocks):
            for name, (block, fn, reps, _) in legs.items():
                if name in ('host', 'copy') and len(times[name]) >= 3:
                    continue
                times[name].append(block(fn, reps))
        for name, ms in times.items():
            r = dict(what=name, params=label, L=L, dB=db, step=s, shape=[legs[name][3] or (1 if name == 'host' else N), T], starts=S, **summary(ms))
            if name == 'host':
                r['scaled_to_32_clips_ms'] = r['median_ms'] * N
            n = legs[name][3]
            if n:
                r['floor_bytes'] = 4 * n * T
                r['design_bytes'] = n * (28 * T + 2 * S)
                r['floor_fraction_of_8TBps'] = r['floor_bytes'] / (r['median_ms'] * 1e-3) / 8e12
                r['design_fraction_of_8TBps'] = r['design_bytes'] / (r['median_ms'] * 1e-3) / 8e12
            rows.append(r)
    for r in rows:
        print('%-11s %-13s %-14s median %10.4f ms   min %10.4f   max %10.4f   (%d blocks)%s%s' % (
            r['what'], r['params'], tuple(r['shape']), r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   floor %.1f %%, design bytes %.1f %% of 8 TB/s' % (100 * r['floor_fraction_of_8TBps'], 100 * r['design_fraction_of_8TBps'])
            if 'floor_bytes' in r else '',
            '   x 32 = %.1f ms' % r['scaled_to_32_clips_ms'] if 'scaled_to_32_clips_ms' in r else ''))
    line = json.dumps({'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'rows': rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
