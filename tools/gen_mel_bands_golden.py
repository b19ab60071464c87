#!/usr/bin/env python
"""Record tests/golden/mel_bands_<case>_{in,gmag,gest}.npz from the mel kernels of the CURRENT build (needs a GPU): the inputs of
tests/test_gpu_mel_bands.py and lin / out of mel_forward_nfk, gmag of mel_backward_nfk (= mel_backward transposed, checked here), gest of
psnd_mel_l1_bwd_nfk.  Run it on the commit whose bits are to be pinned (the fixtures in the tree were recorded at the parent of the
commit that resized the mel kernels' work to the filter bands).

For every clip length of a case that is shorter than the recorded one, the outputs of the current build are checked to be the first
frames of the recorded outputs, bit for bit - the test compares those lengths with the prefix.

usage: tools/gen_mel_bands_golden.py [output directory, default tests/golden]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_mel_bands as T  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else T.GOLD
os.makedirs(out_dir, exist_ok=True)
DEV = T.DEV
for name, c in T.CASES.items():
    from pytorch_sound_amd import kernels as K
    W, mag, gout = T.case_inputs(name)
    M, K_ = W.shape
    log = c['log']
    plan = K.mel_plan(W).to(DEV)
    mag_t, gout_t = torch.from_numpy(mag).to(DEV), torch.from_numpy(gout).to(DEV)
    lin, out = T.run_forward(plan, M, mag_t, log)
    rs = np.random.RandomState(M)
    ref = out.cpu().numpy() + 0.5 * rs.randn(*out.shape).astype(np.float32)
    ref.reshape(-1)[::7] = out.cpu().numpy().reshape(-1)[::7]                 # y == ref: sign 0
    ref_t = torch.from_numpy(ref).to(DEV)
    g_nfk, g_nkf, gest = T.run_backward(plan, K_, gout_t, lin, ref_t, log)
    assert torch.equal(g_nfk.transpose(1, 2).contiguous().view(torch.int32), g_nkf.view(torch.int32)), name
    for t in (lin, g_nfk, gest):
        assert not bool(torch.isnan(t).any()), name
    for F_ in c['Fs']:
        if F_ == c['F']:
            continue
        l2, o2 = T.run_forward(plan, M, mag_t[:, :F_].contiguous(), log)
        cut = lambda t: t[:, :, :F_].contiguous()   # noqa: E731
        a2, b2, e2 = T.run_backward(plan, K_, cut(gout_t), cut(lin), cut(ref_t), log)
        for x, y in ((l2, lin[:, :, :F_]), (o2, out[:, :, :F_]), (a2, g_nfk[:, :F_]), (b2, g_nfk[:, :F_].transpose(1, 2)), (e2, gest[:, :F_])):
            assert T.same_bits(x, y), (name, F_)
    files = {
        'in': dict(W=W, mag_bits16=T.bits16(mag), gout=gout, ref=ref, lin=lin.cpu().numpy(), out=out.cpu().numpy()),
        'gmag': dict(gmag=g_nfk.cpu().numpy()),
        'gest': dict(gest=gest.cpu().numpy()),
    }
    for part, arrays in files.items():
        path = os.path.join(out_dir, 'mel_bands_%s_%s.npz' % (name, part))
        np.savez_compressed(path, **arrays)
        size = os.path.getsize(path)
        assert size < (1 << 20), (path, size)
        print('%s: %d bytes' % (path, size))
    y = out.cpu().numpy()
    print('%s: %d / %d outputs on the low / high clamp of %d, %d non-zero gmag, %d non-zero gest' % (
        name, int((y == np.float32(log[2])).sum()), int((y == np.float32(log[3])).sum()), y.size, int((g_nfk != 0).sum()), int((gest != 0).sum())))
