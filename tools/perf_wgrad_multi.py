#!/usr/bin/env python
"""psnd_conv1d_cl_wgrad_multi alone: 24 convs of the config-2 body (256 -> 256 channels, 3 taps, 32 clips x 173 frames), row ranges per conv
from PSND_WGRAD_MULTI_BLOCKS, both workgroup numberings side by side (PSND_WGRAD_MULTI_MAP: `linear` = conv after conv, the numbering of
before; `grouped` = the tiles of one (conv, row range) behind one L2, what ships).  Lab library (PSND_LIB picks another build of the ABI).

    tools/perf_wgrad_multi.py [block targets ...] [--map=linear|grouped] [--order=co|ci] [--reps=N] [--flush=MB]

--flush: every timed launch on its own, behind a fill of MB megabytes (the operands start outside L2 / Infinity Cache, as they do in a
training step); without it the launches run back to back over operands the launch before just read.
"""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('PSND_LIB', os.path.join(ROOT, 'pytorch_sound_amd', 'libpsnd_hip_lab.so'))
import torch
from pytorch_sound_amd import _lib
from pytorch_sound_amd._lib import lib, stream_ptr, check
opts = dict(a[2:].split('=', 1) for a in sys.argv[1:] if a.startswith('--'))
maps = [opts['map']] if 'map' in opts else ['linear', 'grouped']
reps = int(opts.get('reps', 20))
flush = int(opts.get('flush', 0))
if 'order' in opts:
    os.environ['PSND_WGRAD_MULTI_ORDER'] = opts['order']
dev = torch.device('cuda:0')
N, L, HP, C, k, n = 32, 173, 5, 256, 3, 24
Lp = (L + 2 * HP + 7) // 8 * 8
g = [torch.randn(N, Lp, C, device=dev).to(torch.bfloat16) for _ in range(n)]
x = [torch.randn(N, Lp, C, device=dev).to(torch.bfloat16) for _ in range(n)]
junk = torch.empty(flush << 20, dtype=torch.uint8, device=dev) if flush else None
for blocks in [int(a) for a in sys.argv[1:] if not a.startswith('--')] or [384, 768, 1152, 1536, 2304, 3072]:
    os.environ['PSND_WGRAD_MULTI_BLOCKS'] = str(blocks)
    _lib.refresh_switches()
    S = lib().psnd_conv1d_cl_wgrad_multi_splits(N, Lp, C, C, k, n)
    gw = [torch.empty(S, k, C, C, device=dev) for _ in range(n)]
    gb = [torch.empty(S, C, device=dev) for _ in range(n)]
    arr = (_lib.WgradDesc * n)()
    for i, d in enumerate(arr):
        dil = (1, 1, 3, 1, 5, 1)[i % 6]
        d.g, d.xa, d.gw_part, d.gbias_part, d.off0, d.dstep = g[i].data_ptr(), x[i].data_ptr(), gw[i].data_ptr(), gb[i].data_ptr(), -dil, dil
        d.Ca, d.Cb, d.k, d.splits = C, C, k, S
    run = lambda: check(lib().psnd_conv1d_cl_wgrad_multi(ctypes.addressof(arr), n, N, Lp, stream_ptr(dev)), 'multi')
    us, slabs = {}, {}
    for m in maps:
        os.environ['PSND_WGRAD_MULTI_MAP'] = m
        _lib.refresh_switches()
        for _ in range(3): run()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps if flush else 1)]
        for s, e in ev:
            if flush: junk.fill_(1)
            s.record()
            for _ in range(1 if flush else reps): run()
            e.record()
        torch.cuda.synchronize()
        us[m] = sum(s.elapsed_time(e) for s, e in ev) / reps * 1e3
        slabs[m] = [t.clone() for t in gw + gb]
    same = all(torch.equal(a, b) for a, b in zip(slabs[maps[0]], slabs[maps[-1]]))
    print('target %5d blocks -> %d row ranges per conv, %d workgroups, slabs %.0f MB: %s%s' % (
        blocks, S, 16 * S * n, S * n * k * C * C * 4 / 1e6, '   '.join('%s %.1f us' % (m, us[m]) for m in maps),
        '' if len(maps) < 2 else '   slabs bit-equal: %s' % same), flush=True)
