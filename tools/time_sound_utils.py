"""Times InversePreEmphasis and VolNormConv.forward on a HIP device: the native kernels (psnd_ipreemph_fwd, psnd_volnorm_fwd) against the
path a HIP tensor took before them (torch.nn.RNN = MIOpen's RNN; the python loop over hops), same process, same device, alternating.

    python tools/time_sound_utils.py [--reps 20] [--old-reps 3]

Every path is warmed once at its shape, then timed as host wall time around `reps` calls ending in a device synchronise (VolNormConv's
forward copies the deviations to the host, so its wall time is the honest figure; device events would miss the host loop of the old
path).  Prints one table row per shape and one JSON line.  The outputs of both paths are compared at the timed sizes."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd import kernels as K                                           # noqa: E402
from pytorch_sound_amd.models.sound import InversePreEmphasis, VolNormConv           # noqa: E402


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--old-reps', type=int, default=3)
    ap.add_argument('--T', type=int, default=220500)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda:0')
    rows = []
    ipe = InversePreEmphasis(0.97).to(dev)
    w_ih, w_hh = ipe.rnn.weight_ih_l0.detach(), ipe.rnn.weight_hh_l0.detach()
    for N in (1, 16):
        x = 0.1 * torch.randn(N, 1, a.T, device=dev, generator=torch.Generator(dev).manual_seed(N))
        with torch.no_grad():
            new, y = wall(lambda: ipe(x), a.reps)
            seq, y_seq = wall(lambda: K.InversePreEmphasisFn.apply(x, w_ih, w_hh, K.IPREEMPH_SEQ), a.old_reps)
            try:
                old, y_old = wall(lambda: ipe.rnn(x.transpose(1, 2))[0].transpose(1, 2), a.old_reps)
                diff = (y - y_old).abs().max().item()
            except RuntimeError as e:                                                # the library may refuse the sequence length
                old, diff = None, str(e).splitlines()[0][:120]
        rows.append({'what': 'InversePreEmphasis', 'shape': [N, 1, a.T], 'native_ms': new, 'native_sequential_instance_ms': seq,
                     'previous_ms': old, 'max_abs_diff_vs_previous': diff, 'max_abs_diff_vs_sequential': (y - y_seq).abs().max().item()})
    wav = 0.1 * torch.randn(1, a.T, device=dev, generator=torch.Generator(dev).manual_seed(7))
    vn, vo = VolNormConv(400, 160, -11.5), VolNormConv(400, 160, -11.5)
    vo._native = lambda w: False                                                     # the loop over hops, as before the kernels
    new, out = wall(lambda: vn.forward(wav), a.reps)
    old, out_old = wall(lambda: vo.forward(wav), a.old_reps)
    rel = ((out - out_old).abs() / out_old.abs().clamp_min(1e-7)).max().item()
    rows.append({'what': 'VolNormConv(400, 160, -11.5).forward', 'shape': [1, a.T], 'native_ms': new, 'previous_ms': old,
                 'max_rel_diff_vs_previous': rel, 'std_buffer_max_rel_diff': ((vn.std_buffer - vo.std_buffer).abs() / vo.std_buffer).max().item()})
    for r in rows:
        print('%-40s %-18s native %10.3f ms   previous %s ms' % (r['what'], tuple(r['shape']), r['native_ms'],
                                                                 '%10.3f' % r['previous_ms'] if r['previous_ms'] is not None else 'failed'))
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'rows': rows}))


if __name__ == '__main__':
    main()
