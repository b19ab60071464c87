#!/usr/bin/env python
"""Record tests/golden/wnorm_rows_<case>.npz from the weight-norm backward kernels of the CURRENT build (needs a GPU): g_v, g_g and g_bias
of every conv of every case of tests/test_gpu_wnorm_bwd_rows.py (the inputs come from the seeds there).  Run it on the commit whose bits
are to be pinned (the fixtures in the tree were recorded at the parent of the commit that gave the lean path eight channels per
workgroup).  The single-conv cases are also run as a psnd_conv1d_wnorm_bwd_multi launch of one and checked to give the same bits.

usage: tools/gen_wnorm_bwd_golden.py [output directory, default tests/golden]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_gpu_wnorm_bwd_rows as T  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else T.GOLD
os.makedirs(out_dir, exist_ok=True)
for name in sorted(T.CASES):
    res = T.run_case(name)
    if T.CASES[name][0] == 'single':
        for (gv, gg, gb), (gv2, gg2, gb2) in zip(res, T.run_case(name, 'multi')):
            assert T.same_bits(gv, gv2) and T.same_bits(gg, gg2) and (gb is None or T.same_bits(gb, gb2)), name
    arrays = {}
    for i, (gv, gg, gb) in enumerate(res):
        arrays['gv%d' % i], arrays['gg%d' % i] = gv, gg
        if gb is not None:
            arrays['gb%d' % i] = gb
    path = os.path.join(out_dir, 'wnorm_rows_%s.npz' % name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < (1 << 20), (path, size)
    print('%s: %d bytes, %d convs' % (path, size, len(res)))
