"""Times the sample-rate conversion of psnd_resample.hip on a HIP device against its neighbours, same process, same device, alternating.

    python tools/time_resample.py [--blocks 7] [--reps 20] [--out FILE]

Shapes: 32 clips x 30 s, 44 100 -> 22 050 Hz (1 / 2, 41 taps), 22 050 -> 16 000 Hz (320 / 441, 8821 taps, 28 products per output), and
22 050 -> 44 100 Hz (2 / 1) for the dense comparison.  Legs per shape:
    forward      utils.sound.resample under no_grad: one launch
    fwd+bwd      the same with the input gradient: the kernel twice, the second time with the factors exchanged and the taps reversed
    dense        1 / 2 and 2 / 1 only: the same sum as F.conv1d (stride 2) / F.conv_transpose1d (stride 2) with the 41 taps as one dense
                 filter, through the framework's convolution library.  At 320 / 441 the dense form is a transposed convolution by 320 - a
                 signal 320 times as long, 19 of every 20 products with a stuffed zero - followed by a stride-441 convolution with 8821
                 taps: 6.8e9 samples in between for this shape.  It is not run.
    host         what a user does today with a device tensor: copy to the host, scipy.signal.resample_poly, copy back (wall time)

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed launches of its own leg, then times `reps` calls between
two device events (host: a wall clock around calls that end in a synchronise).  Per leg: the median over the blocks and their spread, and
for the kernel legs the bytes that have to move - 4 (T + T_out) per row and direction - over the time as a fraction of 8 TB/s.
The device outputs are compared with scipy at the timed size."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402
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


def dense(x, up, down, w):
    """the same sum through the convolution library, for 1 / 2 and 2 / 1: w is the (1, 1, taps) filter (symmetric, so no flip)"""
    P = w.shape[-1] // 2
    if (up, down) == (1, 2):
        return F.conv1d(x.unsqueeze(1), w, stride=2, padding=P).squeeze(1)
    return F.conv_transpose1d(x.unsqueeze(1), w, stride=2).squeeze(1)[:, P:P + 2 * x.shape[-1]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    N, rows = 32, []
    for orig_sr, new_sr in ((44100, 22050), (22050, 16000), (22050, 44100)):
        up, down = K.resample_ratio(orig_sr, new_sr)
        T = 30 * orig_sr
        x = 0.1 * torch.randn(N, T, device=dev, generator=torch.Generator(dev).manual_seed(orig_sr))
        xg = x.clone().requires_grad_(True)
        T_out = -(-T * up // down)
        g = torch.randn(N, T_out, device=dev, generator=torch.Generator(dev).manual_seed(new_sr))
        w = K.resample_plan(up, down).on(dev).reshape(1, 1, -1)

        def forward():
            with torch.no_grad():
                return snd.resample(x, orig_sr, new_sr)

        def both():
            return torch.autograd.grad(snd.resample(xg, orig_sr, new_sr), xg, g)[0]

        def host():
            from scipy.signal import resample_poly
            return torch.from_numpy(resample_poly(x.cpu().numpy(), up, down, axis=-1).astype(np.float32)).to(dev)

        legs = {'forward': (device_block, forward, a.reps, 1), 'fwd+bwd': (device_block, both, max(a.reps // 2, 2), 2)}
        if max(up, down) == 2:
            legs['dense'] = (device_block, lambda: dense(x, up, down, w), max(a.reps // 2, 2), 0)
        legs['host'] = (wall_block, host, 1, 0)
        from scipy.signal import resample_poly
        want = torch.from_numpy(resample_poly(x.cpu().double().numpy(), up, down, axis=-1)).to(dev)      # the yardstick in float64
        scale = want.abs().max().item()
        for name in ('forward', 'dense'):
            if name in legs:
                err = (legs[name][1]().double() - want).abs().max().item() / scale
                assert err <= 2.0 ** -20, (name, up, down, err)
        times = {k: [] for k in legs}
        for _ in range(a.blocks):
            for name, (block, fn, reps, _) in legs.items():
                if name == 'host' and len(times[name]) >= 3:              # seconds per call: three blocks are enough
                    continue
                times[name].append(block(fn, reps))
        for name, ms in times.items():
            r = dict(what=name, ratio='%d/%d' % (up, down), shape=[N, T], out_len=T_out, **summary(ms))
            passes = legs[name][3]
            if passes:
                r['bytes'] = passes * 4 * N * (T + T_out)
                r['fraction_of_8TBps'] = r['bytes'] / (r['median_ms'] * 1e-3) / 8e12
            rows.append(r)
        del x, xg, g, want
    for r in rows:
        print('%-8s %-8s %-15s median %9.4f ms   min %9.4f   max %9.4f   (%d blocks)%s' % (
            r['what'], r['ratio'], tuple(r['shape']), r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   %.1f %% of 8 TB/s at 4 (T + T_out) B per row and direction' % (100 * r['fraction_of_8TBps']) if 'bytes' in r else ''))
    line = json.dumps({'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'rows': rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
