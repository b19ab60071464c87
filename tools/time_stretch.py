"""Times the phase vocoder of psnd_phase_vocoder.hip on a HIP device against its neighbours, same process, same device, alternating.

    python tools/time_stretch.py [--blocks 5] [--reps 20] [--out FILE]
    python tools/time_stretch.py --one-clip [--reps 20]   # nothing but one-clip native calls: the run to put under a kernel trace

Shape: 32 clips x 30 s at 22.05 kHz, n_fft 1024, hop 256: (32, 513, 2584) spectra, 0.68 GB read plus written at rate 0.9; and one such
clip (513 rows).  Rates 0.9 and 1.1.  Legs per shape and rate:
    native   kernels.phase_vocoder: one launch
    torch    the same definition in library ops on the device, float32: hypot, atan2, index_select, subtract, cumsum, polar
    host     kernels.phase_vocoder_host (float64 numpy) on one clip's spectrum already in host memory, wall time; times 32 for the batch
    copy     what a user without the native path does first: both parts of the batch to the host (wall time)
    stretch  the whole utils.sound.time_stretch on the waveforms (STFT, vocoder, inverse STFT, trim)
    shift    the whole utils.sound.pitch_shift(+2 semitones) (rate 0.9 only: its own ratio 49 / 55 sets the stretch)

The legs run in alternating blocks.  Every block starts with >= 150 ms of untimed calls of its own leg, then times `reps` calls between two
device events (host, copy: a wall clock).  Per leg the median over the blocks and their spread.  For the native leg the traffic of
8 (F + J) bytes per row as a fraction of 8 TB/s.  The native result is compared with the library-op leg (float32 with a float32 cumsum:
it drifts) and, on clip 0, with the float64 host restatement."""
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
from pytorch_sound_amd.models.transforms import STFT                                 # noqa: E402

SR, N_FFT, HOP = 22050, 1024, 256
HBM = 8.0e12


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


def torch_pv(re, im, rate):
    """the definition of include/psnd.h in library ops, float32 throughout"""
    F = re.shape[-1]
    J = K.pv_frames(F, rate)
    t = torch.arange(J, device=re.device, dtype=torch.float64) * rate
    i = t.floor().long()
    alpha = (t - i).float()
    rp, ip = torch.nn.functional.pad(re, (0, 1)), torch.nn.functional.pad(im, (0, 1))
    mag, ang = torch.hypot(rp, ip), torch.atan2(ip, rp)
    a0, a1 = ang.index_select(-1, i), ang.index_select(-1, i + 1)
    phi = torch.cat((ang[..., :1], a1[..., :-1] - a0[..., :-1]), dim=-1).cumsum(dim=-1)
    m = (1.0 - alpha) * mag.index_select(-1, i) + alpha * mag.index_select(-1, i + 1)
    y = torch.polar(m, phi)
    return y.real, y.imag


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--blocks', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--one-clip', action='store_true', help='only one-clip native calls, for a kernel trace')
    ap.add_argument('--out', default=None, help='also write the JSON line to this file')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    N, T = 32, 30 * SR
    x = clips(N, T, dev)
    stft = STFT(N_FFT, HOP)
    re, im = stft.transform_complex(x)
    re1, im1 = re[:1].contiguous(), im[:1].contiguous()
    Kb, F = re.shape[1], re.shape[2]
    if a.one_clip:
        for _ in range(a.reps):
            K.phase_vocoder(re1, im1, 0.9)
        torch.cuda.synchronize()
        return
    hre, him = re[0].double().cpu().numpy(), im[0].double().cpu().numpy()
    rows, agree = [], {}
    for rate in (0.9, 1.1):
        J = K.pv_frames(F, rate)
        native = K.phase_vocoder(re, im, rate)
        lib = torch_pv(re, im, rate)
        host = K.phase_vocoder_host(hre, him, rate)
        agree['rate %g' % rate] = {
            'native_vs_torch_rel': max(rel(native[0], lib[0]), rel(native[1], lib[1])),
            'native_vs_host_rel_clip0': max(rel(native[0][0].double().cpu(), torch.from_numpy(host[0])),
                                            rel(native[1][0].double().cpu(), torch.from_numpy(host[1])))}
        assert agree['rate %g' % rate]['native_vs_host_rel_clip0'] < 1e-3, agree
        del lib, native
        for label, (r_, i_, xs), n in (('32 clips', (re, im, x), N), ('1 clip', (re1, im1, x[:1].contiguous()), 1)):
            legs = {
                'native': (device_block, lambda: K.phase_vocoder(r_, i_, rate), a.reps),
                'torch': (device_block, lambda: torch_pv(r_, i_, rate), max(a.reps // 4, 2) if n > 1 else a.reps),
                'stretch': (device_block, lambda: U.time_stretch(xs, rate, N_FFT, HOP), max(a.reps // 2, 2)),
            }
            if rate == 0.9:
                legs['shift'] = (device_block, lambda: U.pitch_shift(xs, SR, 2, 12, N_FFT, HOP), max(a.reps // 2, 2))
            if n > 1:
                legs['host'] = (wall_block, lambda: K.phase_vocoder_host(hre, him, rate), 1)
                legs['copy'] = (wall_block, lambda: (re.cpu(), im.cpu()), 2)
            times = {k: [] for k in legs}
            for _ in range(a.blocks):
                for name, (block, fn, reps) in legs.items():
                    if name in ('host', 'copy') and len(times[name]) >= 2:
                        continue
                    times[name].append(block(fn, reps))
            for name, ms in times.items():
                r = dict(what=name, rate=rate, shape=[1 if name == 'host' else n, Kb, F], frames_out=J, **summary(ms))
                if name == 'host':
                    r['scaled_to_32_clips_ms'] = r['median_ms'] * N
                if name == 'native':
                    r['bytes'] = 8 * n * Kb * (F + J)
                    r['fraction_of_8_TB_per_s'] = r['bytes'] / (r['median_ms'] * 1e-3) / HBM
                rows.append(r)
            nat, lib_ms = times['native'], times['torch']
            rows.append(dict(what='native faster than torch in every block', rate=rate, shape=[n, Kb, F],
                             value=all(p < q for p, q in zip(nat, lib_ms)),
                             speedup_of_medians=summary(lib_ms)['median_ms'] / summary(nat)['median_ms']))
    for r in rows:
        if 'median_ms' not in r:
            print('%-40s rate %-4g %-16s %s   (medians: %.1f x)' % (r['what'], r['rate'], tuple(r['shape']), r['value'], r['speedup_of_medians']))
            continue
        print('%-8s rate %-4g %-16s median %10.4f ms   min %10.4f   max %10.4f   (%d blocks)%s%s' % (
            r['what'], r['rate'], tuple(r['shape']), r['median_ms'], r['min_ms'], r['max_ms'], r['blocks'],
            '   %.3f of 8 TB/s' % r['fraction_of_8_TB_per_s'] if 'bytes' in r else '',
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
