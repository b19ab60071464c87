"""bench.py on one GPU, as a plain run: one JSON line with the headline fields only (what --full adds is absent), `--steps` is the number of
timed steps, and `--dump-outputs DIR` writes the last timed step's loss, updated parameters and gradients as float32 .npy, 64 MB at most."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(300)
def test_plain_line_and_dumped_outputs(tmp_path):
    out_dir = tmp_path / 'out'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '2', '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['steps'] == 4 and out['warmup'] == 2 and out['n_gpus'] == 1
    assert out['metric'] == 'audio-sec/s STFT+mel+fwd/bwd' and out['unit'] == 'audio-s/s'
    assert out['higher_is_better'] is True and out['dtype'] == 'bf16'
    assert math.isfinite(out['ms_per_step']) and out['ms_per_step'] > 0
    assert abs(out['value'] - 32 * 2.0 / (out['ms_per_step'] * 1e-3)) <= 1e-6 * out['value']
    for k in ('roofline', 'roofline_instep', 'timing', 'h2d_inclusive', 'config3_step', 'config4_step', 'dropin_step', 'cpu_baseline'):
        assert k not in out, k

    files = sorted(os.listdir(out_dir))
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 * 10 ** 6
    arrays = {f[:-4]: np.load(out_dir / f) for f in files}
    assert all(f.endswith('.npy') for f in files)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert arrays['loss'].shape == () and float(arrays['loss']) > 0
    params = {k[len('param.'):]: a for k, a in arrays.items() if k.startswith('param.')}
    grads = {k[len('grad.'):]: a for k, a in arrays.items() if k.startswith('grad.')}
    assert sum(a.size for a in params.values()) == out['config']['model_params']
    assert set(grads) == set(params) and all(grads[k].shape == params[k].shape for k in params)
    assert any(np.abs(a).max() > 0 for a in grads.values())
