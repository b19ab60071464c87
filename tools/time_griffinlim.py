"""Times the Griffin-Lim phase step of psnd_griffinlim.hip and the whole loop on a HIP device against their neighbours, same process, same
device, alternating.

    python tools/time_griffinlim.py [--blocks 5] [--reps 20] [--out FILE]
    python tools/time_griffinlim.py --one-clip [--reps 20]   # nothing but one-clip native steps: the run to put under a kernel trace

Shape: 32 clips x 30 s at 22.05 kHz, n_fft 1024, hop 256: (32, 513, 2584) spectra, 28 bytes per element and step = 1.19 GB; and one such
clip.  momentum 0.99.  Legs per shape:
    native      kernels.griffinlim_step with the previous spectrum, X written over it: one launch
    torch       the same definition in library ops on the device, float32: mul, sub, hypot, add, div, mul
    host        kernels.griffinlim_step_host (float64 numpy) on one clip's planes already in host memory, wall time; times 32 for the batch
    copy        what a user without the native path does first: the five planes of the batch to the host (wall time)
    loop        the whole kernels.griffinlim, 32 iterations, zero first phase
    loop-torch  the same loop with the library-op step between the same native transforms

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed calls of its own leg, then times `reps` calls between two
device events (host, copy: a wall clock).  Per leg the median over the blocks and their spread.  For the native step the traffic of
28 N K F bytes as a fraction of 8 TB/s, and the same figure for the library-op step.  The device launches per iteration are counted with
torch.profiler as (launches of 4 iterations - launches of 2) / 2.  The native step is compared with the library-op step and, on clip 0,
with the float64 host restatement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402
from pytorch_sound_amd.models.transforms import STFT                                 # noqa: E402

SR, N_FFT, HOP = 22050, 1024, 256
HBM = 8.0e12
MOMENTUM = 0.99
ALPHA = MOMENTUM / (1.0 + MOMENTUM)
N_ITER = 32


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
    """a few gliding partials and a noise floor per clip"""
    g = torch.Generator(dev).manual_seed(SR)
    t = torch.arange(T, device=dev, dtype=torch.float64) / SR
    x = 0.02 * torch.randn(N, T, device=dev, generator=g)
    for h in range(1, 6):
        base = h * (110.0 + 330.0 * torch.rand(N, 1, device=dev, generator=g, dtype=torch.float64))
        f = base * (1.0 + 0.02 * torch.sin(2 * np.pi * 3.0 * t + 6.28 * torch.rand(N, 1, device=dev, generator=g, dtype=torch.float64)))
        x += (torch.sin(2 * np.pi * torch.cumsum(f, dim=1) / SR) / (2.0 * h)).float()
    return x


def torch_step(S, cr, ci, pr, pi, alpha, eps=K.GL_EPS):
    """the definition of include/psnd.h in library ops, float32 throughout"""
    tr, ti = cr - alpha * pr, ci - alpha * pi
    den = torch.hypot(tr, ti) + eps
    return S * (tr / den), S * (ti / den)


def torch_loop(S, stft, n_iter, momentum):
    """kernels.griffinlim with a zero first phase, the step in library ops between the same native transforms"""
    alpha = momentum / (1.0 + momentum)
    with torch.no_grad():
        X, P = K.griffinlim_start(S), None
        for _ in range(n_iter):
            C = stft.transform_complex(stft.inverse_complex(X[0], X[1]))
            if P is None:
                den = torch.hypot(C[0], C[1]) + K.GL_EPS
                X = (S * (C[0] / den), S * (C[1] / den))
            else:
                X = torch_step(S, C[0], C[1], P[0], P[1], alpha)
            P = C
        return stft.inverse_complex(X[0], X[1])


def launches(fn):
    """device kernels launched by fn(), counted by torch.profiler; None where the profiler gives nothing"""
    try:
        from torch.profiler import profile, ProfilerActivity
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith('CUDA') and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n or None
    except Exception as e:                                   # the figure is a by-product: the timings do not depend on it
        print('launch count unavailable: %r' % (e,))
        return None


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--one-clip', action='store_true', help='only one-clip native steps, for a kernel trace')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    N, T = 32, 30 * SR
    stft = STFT(N_FFT, HOP)
    x = clips(N, T, dev)
    re, im = stft.transform_complex(x)
    S = torch.hypot(re, im)
    del x
    # a realistic pair (C, P): the spectra of two consecutive iterations of the loop itself
    X = K.griffinlim_start(S)
    pr, pi = stft.transform_complex(stft.inverse_complex(X[0], X[1]))
    X = K.griffinlim_step(S, pr, pi)
    cr, ci = stft.transform_complex(stft.inverse_complex(X[0], X[1]))
    del X, re, im
    Kb, F = S.shape[1], S.shape[2]
    one = [t[:1].contiguous() for t in (S, cr, ci, pr, pi)]
    if a.one_clip:
        o = (torch.empty_like(one[0]), torch.empty_like(one[0]))
        for _ in range(a.reps):
            K.griffinlim_step(*one, ALPHA, out=o)
        torch.cuda.synchronize()
        return
    native = K.griffinlim_step(S, cr, ci, pr, pi, ALPHA)
    lib = torch_step(S, cr, ci, pr, pi, ALPHA)
    hostp = [t[0:1].double().cpu().numpy() for t in (S, cr, ci, pr, pi)]
    host = K.griffinlim_step_host(*hostp, ALPHA)
    agree = {'native_vs_torch_rel': max(rel(native[0], lib[0]), rel(native[1], lib[1])),
             'native_vs_host_rel_clip0': max(rel(native[0][:1].double().cpu(), torch.from_numpy(host[0])),
                                             rel(native[1][:1].double().cpu(), torch.from_numpy(host[1])))}
    assert agree['native_vs_host_rel_clip0'] < 1e-5, agree
    del native, lib
    rows = []
    for label, planes, n in (('32 clips', (S, cr, ci, pr, pi), N), ('1 clip', one, 1)):
        s_, c0, c1, p0, p1 = planes
        out = (torch.empty_like(s_), torch.empty_like(s_))
        loop_reps = max(a.reps // 8, 2) if n > 1 else max(a.reps // 2, 2)
        legs = {
            'native': (device_block, lambda: K.griffinlim_step(s_, c0, c1, p0, p1, ALPHA, out=out), a.reps),
            'torch': (device_block, lambda: torch_step(s_, c0, c1, p0, p1, ALPHA), max(a.reps // 2, 2) if n > 1 else a.reps),
            'loop': (device_block, lambda: K.griffinlim(s_, stft, N_ITER, MOMENTUM, rand_init=False), loop_reps),
            'loop-torch': (device_block, lambda: torch_loop(s_, stft, N_ITER, MOMENTUM), loop_reps),
        }
        if n > 1:
            legs['host'] = (wall_block, lambda: K.griffinlim_step_host(*hostp, ALPHA), 1)
            legs['copy'] = (wall_block, lambda: [t.cpu() for t in planes], 2)
        times = {k: [] for k in legs}
        for _ in range(a.blocks):
            for name, (block, fn, reps) in legs.items():
                if name in ('host', 'copy') and len(times[name]) >= 2:
                    continue
                times[name].append(block(fn, reps))
        per_iter = {}
        for name, fn in (('loop', lambda k: K.griffinlim(s_, stft, k, MOMENTUM, rand_init=False)), ('loop-torch', lambda k: torch_loop(s_, stft, k, MOMENTUM))):
            n4, n2 = launches(lambda: fn(4)), launches(lambda: fn(2))
            per_iter[name] = None if n4 is None or n2 is None else (n4 - n2) / 2.0
        for name, ms in times.items():
            r = dict(what=name, shape=[1 if name == 'host' else n, Kb, F], **summary(ms))
            if name == 'host':
                r['scaled_to_32_clips_ms'] = r['median_ms'] * N
            if name in ('native', 'torch'):
                r['bytes'] = 28 * n * Kb * F
                r['fraction_of_8_TB_per_s'] = r['bytes'] / (r['median_ms'] * 1e-3) / HBM
            if name in per_iter:
                r['iterations'] = N_ITER
                r['launches_per_iteration'] = per_iter[name]
            rows.append(r)
        for fast, slow in (('native', 'torch'), ('loop', 'loop-torch')):
            rows.append(dict(what='%s faster than %s in every block' % (fast, slow), shape=[n, Kb, F],
                             value=all(p < q for p, q in zip(times[fast], times[slow])),
                             speedup_of_medians=summary(times[slow])['median_ms'] / summary(times[fast])['median_ms']))
    for r in rows:
        if 'median_ms' not in r:
            print('%-44s %-16s %s   (medians: %.2f x)' % (r['what'], tuple(r['shape']), r['value'], r['speedup_of_medians']))
            continue
        print('%-10s %-16s median %10.4f ms   min %10.4f   max %10.4f   (%d blocks)%s%s%s' % (
            r['what'], tuple(r['shape']), r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   %.3f of 8 TB/s' % r['fraction_of_8_TB_per_s'] if 'bytes' in r else '',
            '   x 32 = %.1f ms' % r['scaled_to_32_clips_ms'] if 'scaled_to_32_clips_ms' in r else '',
            '   %s launches per iteration' % r['launches_per_iteration'] if 'launches_per_iteration' in r else ''))
    print(agree)
    line = json.dumps({'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'agreement': agree, 'rows': rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
