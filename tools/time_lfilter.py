"""Times the recursive filter of psnd_lfilter.hip on a HIP device against its neighbours, same process, same device, alternating.

    python tools/time_lfilter.py [--blocks 7] [--reps 20] [--out FILE]

Shape 1: 16 clips x 10 s at 22 050 Hz (the inference shape of the sibling kernel).  Legs:
    parallel     utils.sound.inv_preemphasis on the parallel instance (two launches: span carries, then the walk that stores)
    sequential   the same filter on the sequential instance (one lane per clip)
    sibling      models.sound.InversePreEmphasis, the tanh RNN of psnd_sound.hip - another function, the yardstick for what a latency-bound
                 scan of this geometry costs
    host         what the reference does with a device tensor: copy to the host, scipy.signal.lfilter, copy back (wall time)
Shape 2: 32 clips x 30 s at 44 100 Hz, parallel instance; its 8 bytes per sample (one read, one write; the kernel reads x a second time in
the carry launch) over the time, as a fraction of 8 TB/s.

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed launches of its own leg, then times `reps` calls between
two device events (host: a wall clock around calls that end in a synchronise).  Per leg: the median over the blocks and their spread.
The device outputs are compared with scipy at the timed size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402
from pytorch_sound_amd.models.sound import InversePreEmphasis                        # noqa: E402
from pytorch_sound_amd.utils import sound as snd                                     # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    b, den = [1.0], [1.0, -0.97]
    N, T = 16, 220500
    x = 0.1 * torch.randn(N, T, device=dev, generator=torch.Generator(dev).manual_seed(1))
    ipe = InversePreEmphasis(0.97).to(dev)
    x3 = x.reshape(N, 1, T)

    def host():
        from scipy.signal import lfilter
        return torch.from_numpy(lfilter(b, den, x.cpu().numpy()).astype(np.float32)).to(dev)

    with torch.no_grad():
        legs = {
            'parallel': (device_block, lambda: snd.inv_preemphasis(x), a.reps),
            'sequential': (device_block, lambda: K.lfilter(x, b, den, instance=K.LFILTER_SEQ), max(a.reps // 4, 2)),
            'sibling': (device_block, lambda: ipe(x3), a.reps),
            'host': (wall_block, host, 2),
        }
        assert K.lfilter_instance(b, den) == K.LFILTER_PARALLEL
        want = host().double()
        for name in ('parallel', 'sequential'):
            err = (legs[name][1]().double() - want).abs().max().item() / want.abs().max().item()
            assert err <= 2.0 ** -22, (name, err)
        times = {k: [] for k in legs}
        for _ in range(a.blocks):
            for name, (block, fn, reps) in legs.items():
                times[name].append(block(fn, reps))
        rows = [dict(what=name, shape=[N, T], **summary(ms)) for name, ms in times.items()]
        N2, T2 = 32, 30 * 44100
        x2 = 0.1 * torch.randn(N2, T2, device=dev, generator=torch.Generator(dev).manual_seed(2))
        big = summary([device_block(lambda: snd.inv_preemphasis(x2), max(a.reps // 2, 2)) for _ in range(a.blocks)])
        nbytes = 8 * N2 * T2
        rows.append(dict(what='parallel', shape=[N2, T2], bytes=nbytes, **big,
                         fraction_of_8TBps=nbytes / (big['median_ms'] * 1e-3) / 8e12))
    for r in rows:
        print('%-11s %-16s median %9.4f ms   min %9.4f   max %9.4f   (%d blocks)%s' % (
            r['what'], tuple(r['shape']), r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   %.1f %% of 8 TB/s at 8 B per sample' % (100 * r['fraction_of_8TBps']) if 'bytes' in r else ''))
    line = json.dumps({'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'rows': rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
