"""Times the separation metrics of psnd_separation.hip on a HIP device against their neighbours, same process, same device, alternating.

    python tools/time_sep_metrics.py [--blocks 5] [--reps 10] [--out FILE]
    python tools/time_sep_metrics.py --one-shape [--reps 20]   # nothing but native forward + backward calls at (32, 4, 30 s): for a kernel trace
    python tools/time_sep_metrics.py --count-launches          # kernels per call of the native and the composed path (torch.profiler)

Shapes: (32, 2, 4 s at 16 kHz) and (32, 4, 30 s at 44.1 kHz); targets are noise at distinct levels, estimate i is a shuffled target plus
noise 20 + 5 i dB down.  The timed objective is -mean SI-SDR (zero mean) under permutation-invariant matching.  Legs, per shape:
    native fwd       kernels.sep_metric_loss: three launches, every sample of the 2 S rows read once, the permutation chosen on the device
    native fwd+bwd   the same and loss.backward() to the estimates (one more launch)
    composed fwd     the same definition from library ops, written as an asteroid-style wrapper writes it: the S x S pair matrix by
                     broadcasting (B, S, 1, T) against (B, 1, S, T), the scores of itertools.permutations stacked, min over them on the device
    composed fwd+bwd with autograd through all of it
    host             kernels.sep_metric_host (float64 numpy) on one item already in host memory, wall time, times 32
    copy             what a user without the native path does first: both batches to the host (wall time)

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed calls of its own leg, then times `reps` calls between
two device events (host, copy: a wall clock).  Per leg the median over the blocks and their spread; for the native forward the bytes of
the floor (4 * 2 S * T per item: every row read once) over time as a fraction of 8 TB/s.  The native values are compared with the
composed ones and with the host restatement at the timed size, the permutations exactly."""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402

SHAPES = {'32x2x4s@16k': (32, 2, 4 * 16000), '32x4x30s@44.1k': (32, 4, 30 * 44100)}
EPS = K.SEP_EPS


def spin(fn, seconds=0.15):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(4):
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


def batch(B, S, T, dev):
    g = torch.Generator(dev).manual_seed(B * S + T)
    level = 0.1 * 0.8 ** torch.arange(S, device=dev, dtype=torch.float32)
    tgt = torch.randn(B, S, T, device=dev, generator=g) * level[None, :, None]
    perm = torch.stack([torch.randperm(S, device=dev, generator=g) for _ in range(B)])
    down = 10.0 ** (-(20.0 + 5.0 * torch.arange(S, device=dev, dtype=torch.float32)) / 20.0)
    shuffled = torch.gather(tgt, 1, perm[:, :, None].expand(B, S, T))
    est = shuffled + torch.randn(B, S, T, device=dev, generator=g) * shuffled.std(dim=-1, keepdim=True) * down[None, :, None]
    return est.contiguous(), tgt.contiguous(), perm


def composed(est, tgt):
    """(loss, values (B, S), permutation (B, S)): zero-mean SI-SDR under PIT from library ops, as an asteroid-style wrapper composes it"""
    S = est.shape[1]
    e, s = est[:, :, None, :], tgt[:, None, :, :]
    e, s = e - e.mean(dim=-1, keepdim=True), s - s.mean(dim=-1, keepdim=True)
    a = ((e * s).sum(dim=-1, keepdim=True) + EPS) / ((s * s).sum(dim=-1, keepdim=True) + EPS)
    scaled = a * s
    pair = 10.0 * torch.log10(((scaled * scaled).sum(dim=-1) + EPS) / (((scaled - e) ** 2).sum(dim=-1) + EPS))      # (B, S, S)
    perms = torch.tensor(list(itertools.permutations(range(S))), device=est.device)                                # (S!, S)
    picked = pair[:, torch.arange(S, device=est.device)[None, :], perms]                                             # (B, S!, S)
    best = (-picked.sum(dim=-1)).argmin(dim=1)
    value = picked[torch.arange(est.shape[0], device=est.device), best]
    return -value.mean(), value, perms[best]


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'Memcpy' not in e.name and 'Memset' not in e.name)


def legs_of(est, tgt):
    ge = est.clone().requires_grad_(True)

    def native_fwd():
        return K.sep_metric_loss(est, tgt, 'si_sdr', True, None, None, True)

    def native_both():
        ge.grad = None
        K.sep_metric_loss(ge, tgt, 'si_sdr', True, None, None, True)[0].backward()

    def composed_fwd():
        with torch.no_grad():
            return composed(est, tgt)

    def composed_both():
        ge.grad = None
        composed(ge, tgt)[0].backward()

    return {'native fwd': native_fwd, 'native fwd+bwd': native_both, 'composed fwd': composed_fwd, 'composed fwd+bwd': composed_both}, ge


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--one-shape', action='store_true', help='only native forward + backward calls at the large shape, for a kernel trace')
    ap.add_argument('--count-launches', action='store_true', help='count the kernels of one call of each device leg and stop')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    if a.one_shape:
        est, tgt, _ = batch(*SHAPES['32x4x30s@44.1k'], dev)
        fn = legs_of(est, tgt)[0]['native fwd+bwd']
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return
    rows, checks, kernels = [], {}, {}
    for shape_name, (B, S, T) in SHAPES.items():
        est, tgt, planted = batch(B, S, T, dev)
        legs, ge = legs_of(est, tgt)
        if a.count_launches:
            kernels[shape_name] = {k: count_kernels(fn) for k, fn in legs.items()}
            continue
        # the two paths compute the same thing
        loss, value, perm, _, flag = legs['native fwd']()
        closs, cvalue, cperm = legs['composed fwd']()
        item0 = (est[0].cpu().numpy(), tgt[0].cpu().numpy())
        host = K.sep_metric_host(item0[0][None], item0[1][None], 'si_sdr', True, None, None, True)
        worst = float((value - cvalue).abs().max())
        assert perm.tolist() == planted.tolist() == cperm.tolist() and float(flag) == 0.0
        assert worst < 1e-2 and float(np.max(np.abs(value[0].cpu().numpy() - host))) < 1e-4, (worst, value[0], host)
        legs['native fwd+bwd']()
        g_native = ge.grad.clone()
        legs['composed fwd+bwd']()
        g_err = float((g_native - ge.grad).abs().max() / ge.grad.abs().max())
        assert g_err < 1e-3, g_err
        checks[shape_name] = {'native_minus_composed_max_db': worst, 'gradient_native_minus_composed_rel': g_err, 'loss': float(loss),
                              'composed_loss': float(closs)}
        plan = {k: (device_block, fn, a.reps if 'native' in k else max(a.reps // 4, 2)) for k, fn in legs.items()}
        plan['host'] = (wall_block, lambda: K.sep_metric_host(item0[0][None], item0[1][None], 'si_sdr', True, None, None, True), 2)
        plan['copy'] = (wall_block, lambda: (est.cpu(), tgt.cpu()), 2)
        times = {k: [] for k in plan}
        for _ in range(a.blocks):
            for name, (block, fn, reps) in plan.items():
                if name in ('host', 'copy') and len(times[name]) >= 3:
                    continue
                times[name].append(block(fn, reps))
        for name, ms in times.items():
            r = dict(what=name, shape=shape_name, dims=[1 if name == 'host' else B, S, T], **summary(ms))
            if name == 'host':
                r['scaled_to_the_batch_ms'] = r['median_ms'] * B
            if name == 'native fwd':
                r['floor_bytes'] = 4 * 2 * S * T * B
                r['floor_fraction_of_8TBps'] = r['floor_bytes'] / (r['median_ms'] * 1e-3) / 8e12
            rows.append(r)
        # the native forward + backward is expected to be the faster one in every block
        checks[shape_name]['native_faster_in_every_block'] = all(n < c for n, c in zip(times['native fwd+bwd'], times['composed fwd+bwd']))
        del est, tgt, ge, legs, plan
        torch.cuda.empty_cache()
    if a.count_launches:
        print(json.dumps({'kernels_per_call': kernels}))
        return
    for r in rows:
        print('%-17s %-15s median %10.4f ms   min %10.4f   max %10.4f   (%d blocks)%s%s' % (
            r['what'], r['shape'], r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   floor %.2f %% of 8 TB/s' % (100 * r['floor_fraction_of_8TBps']) if 'floor_bytes' in r else '',
            '   x batch = %.1f ms' % r['scaled_to_the_batch_ms'] if 'scaled_to_the_batch_ms' in r else ''))
    line = json.dumps({'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'checks': checks, 'rows': rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
