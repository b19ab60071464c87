"""Times the bench-shaped config-2 Trainer step (bench.py: build_step, batch 32 x 2 s, pytorch_sound_amd.optim.Adam, graph_steps = True)
with an LR scheduler attached, on a HIP device:

    scheduler        StepLR attached, the Trainer's defaults (async_scheduler: the rate of a step in flight is chosen on the device)
    scheduler_sync   StepLR attached, async_scheduler = False: the reference's host check between forward and backward, eager launches
                     (what every Trainer with a scheduler ran before async_scheduler; on a checkout without the switch this IS `scheduler`)
    no_scheduler     no scheduler: the step bench.py times

    python tools/time_scheduler_step.py [--steps 200] [--rounds 5] [--warmup 60]

Every variant is a Trainer of its own in the same process; all are warmed (eager warm-up steps, the graph capture, `warmup` further steps),
then timed in alternation: `rounds` blocks of `steps` steps each, host wall time around a block that ends in a device synchronise.  Prints
the mean ms/step over all timed steps and the per-block spread of every variant, then one JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench                                                                         # noqa: E402
from pytorch_sound_amd import optim as poptim                                        # noqa: E402


def build(variant, device, pool):
    Trainer, model = bench.build_step(device, amp=True)
    opt = poptim.Adam(model.parameters(), lr=2e-4, betas=(0.8, 0.99))
    sch = None if variant == 'no_scheduler' else torch.optim.lr_scheduler.StepLR(opt, 1000, 0.5)
    huge = 10 ** 9
    tr = Trainer(model, opt, pool, pool, max_step=huge, valid_max_step=1, save_interval=huge, log_interval=huge,
                 save_dir=tempfile.mkdtemp(prefix='psnd_sched_'), save_prefix=variant, scheduler=sch, seed=1234)
    tr.graph_steps = True
    if variant == 'scheduler_sync':
        tr.async_scheduler = False
    model.train()
    return tr


def run(tr, n):
    for _ in range(n):
        tr.step += 1
        tr.train(tr.step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200, help='steps per timed block')
    ap.add_argument('--rounds', type=int, default=5, help='timed blocks per variant, alternating')
    ap.add_argument('--warmup', type=int, default=60)
    ap.add_argument('--variants', default='scheduler,scheduler_sync,no_scheduler')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    device = torch.device('cuda', 0)
    T = int(bench.SR * bench.CLIP_SECONDS)
    pool = [bench.synth_batch(1234 + 1000 * i, bench.BATCH_PER_GPU, T, device) for i in range(8)]
    names = a.variants.split(',')
    trainers = {v: build(v, device, pool) for v in names}
    for tr in trainers.values():
        run(tr, tr.graph_warmup + 1 + a.warmup)
    torch.cuda.synchronize()
    blocks = {v: [] for v in names}
    for _ in range(a.rounds):
        for v in names:
            tr = trainers[v]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(tr, a.steps)
            torch.cuda.synchronize()
            blocks[v].append((time.perf_counter() - t0) / a.steps * 1e3)
    rows = {}
    for v in names:
        tr = trainers[v]
        if hasattr(tr, 'sync_scheduler'):
            tr.sync_scheduler()
        b = blocks[v]
        rows[v] = {'ms_per_step': sum(b) / len(b), 'block_min_ms': min(b), 'block_max_ms': max(b), 'blocks': b,
                   'captured': any(s.captured for s in getattr(tr, '_graphs', {}).values()),
                   'scheduler_steps': None if tr.scheduler is None else tr.scheduler.last_epoch, 'trainer_steps': tr.step}
        print('%-16s %8.3f ms/step   blocks %.3f .. %.3f   %s' % (v, rows[v]['ms_per_step'], min(b), max(b),
                                                                 'hipGraph replay' if rows[v]['captured'] else 'eager launches'))
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'steps_per_block': a.steps, 'rounds': a.rounds, 'warmup': a.warmup, 'rows': rows}))


if __name__ == '__main__':
    main()
