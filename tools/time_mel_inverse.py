"""Times kernels.mel_inverse (psnd_mel_inverse.hip) and the whole mel_to_wave on a HIP device against their neighbours, same process, same
device, alternating.

    python tools/time_mel_inverse.py [--blocks 5] [--reps 10] [--out FILE]
    python tools/time_mel_inverse.py --one-clip [--reps 10]   # nothing but one-clip native launches: the run to put under a kernel trace

Shape: 32 clips x 30 s at 22.05 kHz, n_fft 1024, hop 256, 80 mel bands: (32, 80, 2584) natural-log mels -> (32, 513, 2584) magnitudes,
n_iter = 64; and one such clip.  Legs per shape:
    native      kernels.mel_inverse: one launch for all 64 iterations
    torch       the same definition in library ops on the device, float32: dense matmuls with A and A^T, sub, clamp, axpy
    host        kernels.mel_inverse_host (float64 numpy) on one clip already in host memory, wall time; times 32 for the batch
    copy        what a user without the native path does first and last: the mels to the host, the magnitudes back (wall time)
    mel_to_wave the whole kernels.mel_to_wave: mel_inverse, then 32 iterations of Griffin-Lim, zero first phase

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed calls of its own leg, then times `reps` calls between two
device events (host, copy: a wall clock).  Per leg the median over the blocks and their spread.  For the native launch the arithmetic of
the definition - per frame and iteration 2 flops per non-zero weight in A z and 2 in A^T r, plus the 6 K of the update - as a fraction of
the fp32 vector peak (256 CUs x 128 lanes x 2 flops x 2.4 GHz = 157.3 TFLOP/s), and its Y + x traffic.  Launches per call are counted with
torch.profiler.  The native result is compared with the library-op form and, on clip 0, with the float64 host restatement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402
from pytorch_sound_amd.models.transforms import STFT, LogMelSpectrogram              # noqa: E402

SR, N_FFT, HOP, MELS = 22050, 1024, 256, 80
N_ITER, GL_ITER = 64, 32
PEAK_FP32_VECTOR = 256 * 128 * 2 * 2.4e9


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


class TorchForm:
    """the definition of include/psnd.h in library ops, float32 throughout; the plan's tables on the device"""

    def __init__(self, plan, dev, log_offset):
        h = plan.host
        self.A = torch.from_numpy(h['A']).to(dev)
        self.At = self.A.t().contiguous()
        self.d = torch.from_numpy(h['d']).float().to(dev)[None, :, None]
        self.cinv = torch.from_numpy(h['cinv']).float().to(dev)[None, :, None]
        self.step, self.beta, self.off = float(h['step']), [float(b) for b in h['beta']], log_offset

    def __call__(self, mel, n_iter):
        b = self.d * (torch.exp(mel) - self.off).clamp_min(0.0)
        x = self.cinv * torch.matmul(self.At, b)
        z = x
        for i in range(n_iter):
            r = torch.matmul(self.A, z) - b
            g = torch.matmul(self.At, r)
            xn = torch.add(z, g, alpha=-self.step).clamp_min(0.0)
            z = torch.add(xn, xn - x, alpha=self.beta[i])
            x = xn
        return x


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
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--one-clip', action='store_true', help='only one-clip native launches, for a kernel trace')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    N, T = 32, 30 * SR
    lm = LogMelSpectrogram(SR, MELS, N_FFT, N_FFT, HOP).to(dev)
    stft = STFT(N_FFT, HOP)
    mel = lm(clips(N, T, dev))
    F = mel.shape[-1]
    plan = K.mel_inverse_plan(lm.mel_filter, N_ITER)
    raw = plan.raw()
    Kb = plan.K
    one = mel[:1].contiguous()
    if a.one_clip:
        for _ in range(a.reps):
            K.mel_inverse(one, plan, N_ITER, K.LOG_E, 1e-6)
        torch.cuda.synchronize()
        return
    form = TorchForm(plan, dev, 1e-6)
    native, lib = K.mel_inverse(mel, plan, N_ITER, K.LOG_E, 1e-6), form(mel, N_ITER)
    host_in = one.double().cpu().numpy()
    host = K.mel_inverse_host(host_in, plan, N_ITER, K.LOG_E, 1e-6)
    agree = {'native_vs_torch_rel': rel(native, lib), 'native_vs_host_rel_clip0': rel(native[:1].double().cpu(), torch.from_numpy(host))}
    assert agree['native_vs_host_rel_clip0'] < 1e-3, agree
    del native, lib
    flops_per_frame_iter = 2.0 * raw['nnz_rows'] + 2.0 * raw['nnz_cols'] + 6.0 * Kb
    rows = []
    for label, y, n in (('32 clips', mel, N), ('1 clip', one, 1)):
        legs = {
            'native': (device_block, lambda: K.mel_inverse(y, plan, N_ITER, K.LOG_E, 1e-6), a.reps),
            'torch': (device_block, lambda: form(y, N_ITER), max(a.reps // 4, 2) if n > 1 else a.reps),
            'mel_to_wave': (device_block, lambda: K.mel_to_wave(y, plan, stft, N_ITER, GL_ITER, 0.99, K.LOG_E, 1e-6, rand_init=False),
                            max(a.reps // 4, 2) if n > 1 else a.reps),
        }
        if n > 1:
            legs['host'] = (wall_block, lambda: K.mel_inverse_host(host_in, plan, N_ITER, K.LOG_E, 1e-6), 1)
            back = torch.zeros(N, Kb, F)
            legs['copy'] = (wall_block, lambda: (y.cpu(), back.to(dev)), 2)
        times = {k: [] for k in legs}
        for _ in range(a.blocks):
            for name, (block, fn, reps) in legs.items():
                if name in ('host', 'copy') and len(times[name]) >= 2:
                    continue
                times[name].append(block(fn, reps))
        counts = {name: launches(legs[name][1]) for name in ('native', 'torch', 'mel_to_wave')}
        for name, ms in times.items():
            r = dict(what=name, shape=[1 if name == 'host' else n, MELS, F], **summary(ms))
            if name == 'host':
                r['scaled_to_32_clips_ms'] = r['median_ms'] * N
            if name == 'native':
                r['flops'] = flops_per_frame_iter * N_ITER * n * F
                r['fraction_of_fp32_vector_peak'] = r['flops'] / (r['median_ms'] * 1e-3) / PEAK_FP32_VECTOR
                r['bytes'] = 4 * n * F * (MELS + Kb)
                r['tile'] = K.mel_inverse_tile(MELS, Kb)
            if name in counts:
                r['launches_per_call'] = counts[name]
            rows.append(r)
        rows.append(dict(what='native faster than torch in every block', shape=[n, MELS, F],
                         value=all(p < q for p, q in zip(times['native'], times['torch'])),
                         speedup_of_medians=summary(times['torch'])['median_ms'] / summary(times['native'])['median_ms']))
    for r in rows:
        if 'median_ms' not in r:
            print('%-44s %-16s %s   (medians: %.2f x)' % (r['what'], tuple(r['shape']), r['value'], r['speedup_of_medians']))
            continue
        print('%-12s %-16s median %10.4f ms   min %10.4f   max %10.4f   (%d blocks)%s%s%s' % (
            r['what'], tuple(r['shape']), r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   %.3f of the fp32 vector peak, tile %d' % (r['fraction_of_fp32_vector_peak'], r['tile']) if 'flops' in r else '',
            '   x 32 = %.1f ms' % r['scaled_to_32_clips_ms'] if 'scaled_to_32_clips_ms' in r else '',
            '   %s launches per call' % r['launches_per_call'] if 'launches_per_call' in r else ''))
    print(agree)
    line = json.dumps({'device': torch.cuda.get_device_name(0), 'reps': a.reps, 'agreement': agree, 'rows': rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
