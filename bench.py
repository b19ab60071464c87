#!/usr/bin/env python
"""bench.py - headline benchmark: audio-seconds/second through one training step
STFT -> mel -> model forward -> backward -> (all-reduce) -> optimizer step on MI355X.

  python bench.py --gpus 1 --steps 20 --warmup 5
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): speech source-separation Conv1d model (VoiceBank-like), 22.05 kHz,
1024-pt STFT / hop 256 / 80 mel, bf16 model, batch = 32 x 2 s clips PER GPU (weak scaling), synthetic
clips resident in HBM, random-init weights.  One "step" = Trainer.train(): zero_grad, forward (two
psnd_stft_fwd launches, the separator under bf16 autocast, psnd_mel_fwd x2), NaN check, backward
(incl. psnd_mel_bwd), flat-bucket RCCL all-reduce overlapped with backward, Adam step.

Prints ONE JSON line on rank 0 (`settle` = untimed set-up steps in front of the warm-up).  A plain run sets up, warms up, times the K
steps and prints the headline fields (metric, value, unit, higher_is_better, dtype, ms_per_step, config).  `--dump-outputs DIR` writes
what the last timed step computed (bench_outputs).  `--full` adds these objects, each measured by runs of its own after the timed steps:
  roofline         the STFT kernel the timed step launches (psnd_stft_mag_nfk: wav -> magnitude (N, F, K), stft_fwd_n1024q_kernel) on a
                   544 MB working set (1024 clips, >> the 256 MiB Infinity Cache): algorithmic bytes 4*N*T + 4*N*K*F per launch / mean
                   launch duration (HIP events on the launch stream, measured in this run) against 8 TB/s; frac_config5 / frac_nkf /
                   frac_config5_nkf beside it
  roofline_nkf     the same transform in the reference's layout (N, K, F) (psnd_stft_fwd, stft_fwd_n1024_kernel)
  roofline_instep  the step's launch as it runs inside the timed steps (64 clips, 34 MB, cache resident): a latency figure
  roofline_config5 BASELINE config 5: n_fft 4096 / hop 1024, 32 clips x 30 s at 44.1 kHz (508 MB), (N, F, K) - stft_fwd_n4096r_kernel;
                   roofline_config5_nkf: the (N, K, F) kernel
  roofline_copy    a plain copy of the same bytes as the judged launch under the same timing (what the box delivers to the simplest kernel)
  roofline_mel     the unfused mel stage; roofline_conv: the conv kernels that take most of the step, against the dense bf16 MFMA peak
  config3_step / config4_step   BASELINE configs[2] / configs[3] on one GPU: ms/step, p50 / p99 / max over 200 steps, fraction of the MFMA peak
  dropin_step      configs[1] written against the reference's API names only (Trainer.forward override, STFT.transform, F.l1_loss)
  h2d_inclusive    the same step with the batches in pinned HOST memory (the reference's loop includes this copy,
                   trainer.py:202): copied on a side stream one step ahead (Trainer.prefetch_prepare) and in line
  cpu_baseline     the reference's CPU path (oracle/torch_ref.py port of its dense-DFT conv1d STFT + mel,
                   same model / loss / optimizer in fp32) timed on this host's cores on a bounded sample;
  cpu_baseline_torch_stft  the same step with the reference's torch.stft front end (STFTTorchAudio) instead
  timing           ms/step of the contract region and of further identical K-step blocks (>= 100 ms timed in all): the spread
`--config 3 | 4 | 5 --gpus N` runs BASELINE configs[2] / [3] / [4] data-parallel under the same contract (config_bench).

  python bench.py --gpus 1 --steps 20 --warmup 5 --full                     # every figure above
  python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs out_dir     # + the last timed step's outputs as .npy
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SR, N_FFT, HOP, N_MEL, FMIN, FMAX = 22050, 1024, 256, 80, 0.0, 8000.0
CLIP_SECONDS = 2.0
BATCH_PER_GPU = 32
MFMA_BF16_PEAK = 2.5e15      # dense bf16 MFMA, MI355X_MICROARCH.md
HBM_PEAK = 8.0e12


def synth_batch(seed, n, t, device):
    """BASELINE.md synthetic input: 0.0708*randn + 440 Hz and 3 kHz sinusoids at 0.1, clipped."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    tt = torch.arange(t, dtype=torch.float32) / SR
    tone = 0.1 * torch.sin(2 * np.pi * 440 * tt) + 0.1 * torch.sin(2 * np.pi * 3000 * tt + 0.3)
    clean = (0.0708 * torch.randn(n, t, generator=g) + tone).clamp(-1, 1)
    noisy = (clean + 0.03 * torch.randn(n, t, generator=g)).clamp(-1, 1)
    # mixture clips then reference clips in ONE (2n, t) tensor: the step's single STFT launch reads it as it is (no torch.cat)
    both = torch.cat([noisy, clean])
    if device.type == 'cpu' and torch.cuda.is_available():
        both = both.pin_memory()
    return (both.to(device),)


def build_step(device, amp, static=True, cpu_frontend='port', fused_loss=True, layout='nfk'):
    """returns (trainer_cls, model) for the config-2 step on `device`.  static: the features go into persistent buffers that the step
    graph reads in place (Trainer.static_prepare) - off when prepare() runs one step ahead on a side stream (--prefetch).
    cpu_frontend (CPU baseline leg only): 'port' = the reference's dense-DFT conv1d STFT, 'torch_stft' = its torch.stft class.
    layout (GPU, fused loss): 'nfk' = the magnitudes stay bin-fastest (N, F, K) between the STFT kernel and their consumers (psnd_stft_mag_nfk,
    the channels-last order of the conv stack: no transposing passes); 'nkf' = the reference's (N, K, F) everywhere (round 3's step)."""
    from pytorch_sound_amd.models import build_model
    from pytorch_sound_amd.models import separator  # noqa: F401  (registers conv_separator)
    from pytorch_sound_amd.trainer import Trainer, LogType

    gpu = device.type == 'cuda'
    if gpu:
        from pytorch_sound_amd.models.transforms import LogMelSpectrogram
        from pytorch_sound_amd import kernels as K
        fe = LogMelSpectrogram(SR, N_MEL, N_FFT, N_FFT, HOP, -50, 30, FMIN, FMAX).to(device)

        feat = {}                                                   # persistent feature buffers (Trainer.static_prepare)
        nfk = layout == 'nfk' and fused_loss

        def magnitude_nfk(w):
            n, t = w.shape
            if not static:
                return K.stft_mag_nfk(w, N_FFT, HOP, fe.stft._plan(w.device), K.FRAMING_CENTER, 0.0)
            key = ('mag_nfk', n, t)
            if key not in feat:
                feat[key] = torch.empty((n, K.frame_count(t, N_FFT, HOP), N_FFT // 2 + 1), dtype=torch.float32, device=w.device)
            return K.stft_mag_nfk(w, N_FFT, HOP, fe.stft._plan(w.device), K.FRAMING_CENTER, 0.0, out=feat[key])

        def logmel_of_mag_nfk(m):
            if not static:
                return K.mel_forward_nfk(m, fe._mel_plan(), N_MEL, K.LOG_E, 1e-6, None, fe.min_db, fe.max_db)[0]
            key = ('mel', m.shape[0], m.shape[1])
            if key not in feat:
                feat[key] = torch.empty((m.shape[0], N_MEL, m.shape[1]), dtype=torch.float32, device=m.device)
            return K.mel_forward_nfk(m, fe._mel_plan(), N_MEL, K.LOG_E, 1e-6, None, fe.min_db, fe.max_db, out=feat[key])[0]

        def magnitude(w):
            n, t = w.shape
            if not static:
                return K.stft_forward(w, N_FFT, HOP, fe.stft._plan(w.device), K.FRAMING_CENTER, 0.0)['mag']
            key = ('mag', n, t)
            if key not in feat:
                feat[key] = torch.empty((n, N_FFT // 2 + 1, K.frame_count(t, N_FFT, HOP)), dtype=torch.float32, device=w.device)
            return K.stft_forward(w, N_FFT, HOP, fe.stft._plan(w.device), K.FRAMING_CENTER, 0.0, out_mag=feat[key])['mag']

        def logmel_of_mag(m, persistent=False):
            if not persistent:
                return K.MelLog.apply(m, fe._mel_plan(), N_MEL, K.LOG_E, 1e-6, None, fe.min_db, fe.max_db)
            if not static:
                return K.mel_forward(m, fe._mel_plan(), N_MEL, K.LOG_E, 1e-6, None, fe.min_db, fe.max_db)[0]
            key = ('mel', m.shape[0], m.shape[2])
            if key not in feat:
                feat[key] = torch.empty((m.shape[0], N_MEL, m.shape[2]), dtype=torch.float32, device=m.device)
            return K.mel_forward(m, fe._mel_plan(), N_MEL, K.LOG_E, 1e-6, None, fe.min_db, fe.max_db, out=feat[key])[0]

        l1 = K.l1_loss                                              # F.l1_loss as psnd_l1_loss_fwd / _bwd
        l1sum = K.l1_loss_sum
    else:
        from oracle.torch_ref import RefLogMel, RefLogMelTorch      # CPU baseline leg only
        fe = (RefLogMelTorch if cpu_frontend == 'torch_stft' else RefLogMel)(SR, N_MEL, N_FFT, N_FFT, HOP, -50, 30, FMIN, FMAX)

        def magnitude(w):
            return fe.stft.transform(w)[0]

        def logmel_of_mag(m, persistent=False):
            return fe.mel_of_mag(m)

        l1 = F.l1_loss
        l1sum = None
        nfk = False

    class StepTrainer(Trainer):
        static_prepare = gpu and static   # the features are written into persistent buffers: the step graph reads them in place

        def prepare(self, both):
            # feature extraction of the batch (no parameters, no gradient): eager, ahead of the captured graph
            with torch.no_grad():
                n = both.shape[0] // 2
                if nfk:
                    mag = magnitude_nfk(both)                     # (2 n, F, K): ONE launch, a frame's spectrum contiguous
                    mag_mix, mag_ref = mag[:n], mag[n:]
                    mel_ref = logmel_of_mag_nfk(mag_ref)
                    return mag_mix, mag_ref, mel_ref
                mag = magnitude(both)                             # mixture and reference clips: ONE STFT launch (2 x batch clips)
                mag_mix, mag_ref = mag[:n], mag[n:]
                mel_ref = logmel_of_mag(mag_ref, persistent=True)
            return mag_mix, mag_ref, mel_ref

        def forward(self, mag_mix, mag_ref, mel_ref, is_logging=False):
            if gpu and fused_loss:
                # mask head + both L1 terms as one node: 4 launches forward, 2 backward (cl.MaskHeadSpectralL1CL)
                with torch.autocast('cuda', dtype=torch.bfloat16, enabled=amp):
                    loss, _ = self.model.spectral_l1_loss(mag_mix, mag_ref, mel_ref, fe._mel_plan(), N_MEL, 1.0, 0.5, 1e-6, fe.min_db,
                                                          fe.max_db, layout='nfk' if nfk else 'nkf')
                self.last_loss = loss.detach()      # the value only (no autograd graph kept alive); captured: every replay rewrites it
                return loss, {'loss': (loss, LogType.SCALAR)}
            if amp:
                with torch.autocast('cuda', dtype=torch.bfloat16):
                    est = self.model(mag_mix)
                est = est.float()
            else:
                est = self.model(mag_mix)
            if l1sum is not None:           # both L1 terms as one scalar node (psnd_l1_loss_sum_fwd)
                loss = l1sum([(est, mag_ref), (logmel_of_mag(est), mel_ref)], (1.0, 0.5))
            else:
                loss = l1(est, mag_ref) + 0.5 * l1(logmel_of_mag(est), mel_ref)
            self.last_loss = loss.detach()
            return loss, {'loss': (loss, LogType.SCALAR)}

    torch.manual_seed(1234)
    model = build_model('conv_separator_voicebank').to(device)
    return StepTrainer, model


DUMP_BYTES = 60 * 10 ** 6        # what --dump-outputs writes at most (data; the .npy headers stay well inside 64 MB)


def _trainer_outputs(tr):
    """what a training step hands its caller: the loss, the updated parameters and the gradients they were updated with"""
    out = {'loss': tr.last_loss} if getattr(tr, 'last_loss', None) is not None else {}
    for name, p in tr._bare_model.named_parameters():
        out['param.' + name] = p
        if p.grad is not None:
            out['grad.' + name] = p.grad
    return out


def bench_outputs(path, arrays):
    """--dump-outputs: every tensor of `arrays` as <path>/<name>.npy in float32.  When they hold more than DUMP_BYTES in all, each is cut
    to the same fraction of its elements, at flat positions drawn from a fixed seed (the same for every run with the same arguments)."""
    os.makedirs(path, exist_ok=True)
    total = sum(4 * t.numel() for t in arrays.values())
    frac = min(1.0, DUMP_BYTES / max(total, 1))
    for name, t in arrays.items():
        a = t.detach().float().reshape(-1).cpu().numpy()
        if frac < 1.0:
            k = max(1, int(a.size * frac))
            a = a[np.unique(np.random.default_rng(0).integers(0, a.size, k))]
        np.save(os.path.join(path, name + '.npy'), a.reshape(t.shape) if frac == 1.0 else a)


def gpu_bench(args):
    from pytorch_sound_amd import distributed as pdist
    from pytorch_sound_amd import kernels as K
    if args.force_ddp and int(os.environ.get('WORLD_SIZE', '1')) <= 1:
        # one-rank RCCL process group: the whole data-parallel step (flat buckets, captured all-reduce, hand-over from inside the
        # backward) on one GPU - what the reducer costs without a second device (the sum over one rank is the identity)
        os.environ.update(PSND_DDP_FORCE='1', MASTER_ADDR='127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29517')
        torch.cuda.set_device(0)
        torch.distributed.init_process_group('nccl', rank=0, world_size=1)
    distributed = pdist.init_from_env('nccl')
    rank, world = pdist.rank(), pdist.world_size()
    if world != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run' % (args.gpus, world))
    local = 0 if os.environ.get('PSND_DIST_SHARE_GPU') == '1' else int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    T = int(SR * CLIP_SECONDS)
    N = BATCH_PER_GPU

    Trainer, model = build_step(device, amp=True, static=not args.prefetch, fused_loss=not args.unfused_loss, layout=args.layout)
    from pytorch_sound_amd import optim as poptim
    # torch.optim.Adam semantics as one HIP launch (psnd_adam_step); --torch-adam keeps torch's fused multi-tensor kernel
    opt = (torch.optim.Adam(model.parameters(), lr=2e-4, betas=(0.8, 0.99), fused=True) if args.torch_adam
           else poptim.Adam(model.parameters(), lr=2e-4, betas=(0.8, 0.99)))
    pool = [synth_batch(1234 + rank + 1000 * i, N, T, device) for i in range(args.pool)]
    save_dir = tempfile.mkdtemp(prefix='psnd_bench_')
    huge = 10 ** 9
    tr = Trainer(model, opt, pool, pool, max_step=huge, valid_max_step=1, save_interval=huge, log_interval=huge,
                 save_dir=save_dir, save_prefix='bench', seed=1234)
    tr.graph_steps = not args.no_graph          # forward + backward replayed as one hipGraph (Trainer.graph_steps)
    if tr._reducer is not None and args.no_handover:
        tr._reducer.sink_enabled = False
    # next batch's feature extraction on a side stream (Trainer.prefetch_prepare): +1.6 % throughput, but the in-step STFT
    # launch then shares the chip with the conv kernels and its event timing doubles - off for the judged line
    tr.prefetch_prepare = args.prefetch
    # the next batch's feature extraction behind this step's backward, on a side stream next to the optimizer launch (Trainer.overlap_prepare)
    tr.overlap_prepare = args.overlap_prepare and not args.prefetch          # measured: no gain (0.691 vs 0.682 ms, the STFT launch doubles next to the optimizer's): off
    model.train()

    def barrier():
        torch.cuda.synchronize()
        if distributed:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    step = 0
    if tr.graph_steps:                  # set-up, like building the model: eager steps + the one-off graph capture
        for _ in range(tr.graph_warmup + 1):
            step += 1
            tr.step = step
            tr.train(step)
    for _ in range(args.settle):        # set-up as well: the first ~30 ms of replays run below the steady clock (timing.blocks shows it)
        step += 1
        tr.step = step
        tr.train(step)
    for _ in range(args.warmup):
        step += 1
        tr.step = step
        tr.train(step)
    barrier()
    if args.full:                       # HIP events around the step's STFT launch, for roofline_instep
        K.STFT_FWD_EVENTS = []
        K.STFT_NFK_EVENTS = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step += 1
        tr.step = step
        tr.train(step)
    torch.cuda.synchronize()
    if distributed:
        torch.distributed.barrier()
        torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if distributed:
        tdt = torch.tensor([dt], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(tdt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tdt.item())
    if args.dump_outputs and rank == 0:
        bench_outputs(args.dump_outputs, _trainer_outputs(tr))
    out = None
    if rank == 0:
        audio_s = world * N * CLIP_SECONDS * args.steps
        out = {
            'metric': 'audio-sec/s STFT+mel+fwd/bwd', 'value': audio_s / dt, 'unit': 'audio-s/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'settle': args.settle, 'ms_per_step': dt / args.steps * 1e3,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': 'bf16', 'data': 'synthetic',
            'config': {'workload': 'configs[1]: Conv1d separator (4 x ResBlock1, C=256, on 513-bin magnitude), '
                                   '22.05 kHz, STFT 1024/256, 80 mel, batch 32 x 2 s per GPU, Adam, bf16 autocast',
                       'global_batch': world * N, 'clip_seconds': CLIP_SECONDS, 'parallelism': 'dp%d' % world,
                       'model_params': sum(p.numel() for p in model.parameters())},
            'settle_note': '`settle` untimed set-up steps (clock ramp) run in front of the `warmup` steps; with --full, timing.blocks_ms_per_step shows what is left of the ramp',
        }
    if args.full:
        extra = _full_figures(args, tr, device, distributed, rank, world, dt, step)
        if out is not None:
            out.update(extra)
    return out, device


def _full_figures(args, tr, device, distributed, rank, world, dt, step):
    """--full: the figures beyond the headline, each from runs of its own behind the timed steps - the spread over further K-step blocks,
    the step with its batches in pinned host memory, the STFT launch inside the timed steps, and on rank 0 the rooflines and the
    single-GPU legs.  Every rank takes part (the blocks are collective); rank 0 gets the line's extra entries, the others None."""
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    T = int(SR * CLIP_SECONDS)
    N = BATCH_PER_GPU

    def barrier():
        torch.cuda.synchronize()
        if distributed:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    instep_nfk = len(K.STFT_NFK_EVENTS) > 0
    ev_instep = K.STFT_NFK_EVENTS if instep_nfk else K.STFT_FWD_EVENTS
    K.STFT_FWD_EVENTS = None
    K.STFT_NFK_EVENTS = None
    # ---- spread: the contract region above is K steps (~17 ms at K = 20); the same K steps are repeated in further timed blocks
    #      (each bracketed like the first) until >= 100 ms have been timed, and every block's ms/step is reported next to `value`
    blocks = [dt / args.steps * 1e3]
    n_blocks = int(min(64, max(4, np.ceil(0.1 / max(dt, 1e-6)))))
    for _ in range(n_blocks):
        barrier()
        tb = time.perf_counter()
        for _ in range(args.steps):
            step += 1
            tr.step = step
            tr.train(step)
        barrier()
        d = time.perf_counter() - tb
        if distributed:
            tdt = torch.tensor([d], device=device, dtype=torch.float64)
            torch.distributed.all_reduce(tdt, op=torch.distributed.ReduceOp.MAX)
            d = float(tdt.item())
        blocks.append(d / args.steps * 1e3)
    timing = {'blocks_ms_per_step': [round(b, 4) for b in blocks], 'block_steps': args.steps, 'blocks': len(blocks),
              'total_timed_ms': float(sum(blocks) * args.steps), 'min': float(min(blocks)), 'median': float(np.median(blocks)),
              'max': float(max(blocks)),
              'note': 'block 0 is the contract region (`ms_per_step`, `value`); the further blocks repeat the same K steps'}

    # ---- the same step with the batches in pinned HOST memory (the reference's loop includes this copy: trainer.py:202,
    #      utils/tensor.py:15).  (a) copied + feature-extracted one step ahead on a side stream (Trainer.prefetch_prepare),
    #      (b) copied in line on the compute stream as the reference does.  Same K steps each, max over ranks.
    h2d = {}
    host_pool = [synth_batch(1234 + rank + 1000 * i, N, T, torch.device('cpu')) for i in range(args.pool)]
    ovl_keep = tr.overlap_prepare
    tr.overlap_prepare = False
    for mode in ('prefetch_copy', 'inline'):
        tr.train_dataset = tr.repeat(host_pool)
        tr._ovl = None                                # (a batch staged by overlap_prepare belongs to the device-resident pool)
        tr.prefetch_prepare = False
        tr.prefetch_copy = mode == 'prefetch_copy'
        tr._pre_stream = None
        for _ in range(3):
            step += 1
            tr.step = step
            tr.train(step)
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step += 1
            tr.step = step
            tr.train(step)
        barrier()
        d = time.perf_counter() - t1
        if distributed:
            tdt = torch.tensor([d], device=device, dtype=torch.float64)
            torch.distributed.all_reduce(tdt, op=torch.distributed.ReduceOp.MAX)
            d = float(tdt.item())
        h2d[mode] = {'value': world * N * CLIP_SECONDS * args.steps / d, 'ms_per_step': d / args.steps * 1e3}
    tr.prefetch_prepare, tr.prefetch_copy = args.prefetch, False
    tr.overlap_prepare = ovl_keep
    h2d['default'] = 'prefetch_copy (Trainer.prefetch_copy = None: on when the batches arrive in pinned host memory)'
    h2d['unit'] = 'audio-s/s'
    h2d['bytes_per_step'] = 2 * N * T * 4
    h2d['note'] = ('batches in pinned host memory, %d steps: "prefetch_copy" = the copy of the next batch on a side stream while the '
                   'step computes (Trainer.prefetch_copy), "inline" = .cuda(non_blocking) on the compute stream as the '
                   'reference\'s Trainer.train does') % args.steps

    # ---- roofline of the STFT kernel as launched in the timed region (rank 0) ------------------------
    Kb = N_FFT // 2 + 1
    Fr = K.frame_count(T, N_FFT, HOP)
    ev = ev_instep
    t_raw = float(np.mean([a.elapsed_time(b) for a, b, _ in ev])) * 1e-3
    # an event pair around NOTHING on a busy stream still reads ~5 us (the two marker packets); on this 12-13 us launch
    # (rocprofv3 kernel time, profiles/) that overhead is reported next to the raw figure, not subtracted - the two
    # do not simply add
    t_ovh = _event_pair_overhead(device)
    t_stft = t_raw
    n_launch = int(ev[0][2])                       # clips per in-step launch (mixture + reference clips of a batch together)
    bytes_launch = 4 * n_launch * T + 4 * n_launch * Kb * Fr
    roofline_instep = {'bound': 'hbm', 'kernel': ('stft_fwd_n1024q_kernel (wav -> magnitude (N,F,K), 1024/256)' if instep_nfk else
                                                  'stft_fwd_n1024_kernel<mag> (wav -> magnitude, 1024/256)'),
                       'achieved': bytes_launch / t_stft / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s',
                       'frac': bytes_launch / t_stft / HBM_PEAK, 'traffic': None,
                       'bytes_per_launch': bytes_launch, 'launch_us': t_stft * 1e6,
                       'empty_event_pair_us': t_ovh * 1e6, 'launches_timed': len(ev),
                       'note': 'the launch inside the timed steps (mixture + reference clips of the batch): 704 workgroups, 34 MB '
                               '(Infinity-Cache resident) - one workgroup lifetime, a latency figure, not a bandwidth measurement'}
    out = None
    if rank == 0:
        # The judged `roofline` is the kernel the timed step launches - psnd_stft_mag_nfk, stft_fwd_n1024q_kernel - on an HBM-sized working
        # set (1024 clips x 2 s: 181 MB in + 363 MB out = 544 MB >> the 256 MiB Infinity Cache), HIP events around every launch, measured in
        # this run; the same transform in the reference's (N, K, F) layout (psnd_stft_fwd, what STFT.transform returns) is `roofline_nkf`,
        # BASELINE config 5 `roofline_config5` (N, F, K) / `roofline_config5_nkf`.
        roofline = _nfk_roofline(device, N_FFT, HOP, 1024, T, 'stft_fwd_n1024q_kernel (a wave owns four frames; wav -> magnitude (N,F,K), 1024/256)')
        roofline['workload'] = ('1024 clips x 2 s, 1024/256: 181 MB in + 363 MB out = 544 MB (> the 256 MiB Infinity Cache): the kernel the timed step '
                                'launches (psnd_stft_mag_nfk, bin-fastest magnitudes for the in-library consumers) on an HBM-sized working set; HIP '
                                'events around every launch, measured in this run')
        NL = 1024
        wav = torch.randn(NL, T, device=device) * 0.07
        plan = K.stft_plan(N_FFT, _hann(N_FFT)).to(device)
        mag = torch.empty(NL, Kb, Fr, device=device)
        mk = _time_launches(lambda: check(lib().psnd_stft_fwd(ptr(wav), NL, T, N_FFT, HOP, 0, ptr(plan), 0.0, ptr(mag), None, None, None,
                                                              stream_ptr(device)), 'psnd_stft_fwd'))
        tl = mk['t']
        bl = 4 * NL * T + 4 * NL * Kb * Fr
        roofline_nkf = {'bound': 'hbm', 'kernel': 'stft_fwd_n1024_kernel<mag> (wav -> magnitude (N,K,F), 1024/256)',
                        'achieved': bl / tl / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s',
                        'frac': bl / tl / HBM_PEAK, 'traffic': _pmc_traffic('n1024'), 'traffic_source': _pmc_traffic('n1024', 'source'),
                        'bytes_per_launch': bl, **_launch_fields(mk),
                        'workload': '1024 clips x 2 s, 1024/256, the reference layout (N, K, F) of STFT.transform: 544 MB; HIP events around every launch'}
        del wav, mag
        roofline_config5_nkf = _config5_roofline(device)
        roofline_config5 = _nfk_roofline(device, 4096, 1024, 32, int(44100 * 30.0),
                                         'stft_fwd_n4096r_kernel (LDS sample ring + loader wave, one wave per frame, stores from registers; wav -> magnitude (N,F,K), 4096/1024)')
        roofline_config5['workload'] = 'configs[4]: 32 clips x 30 s at 44.1 kHz, n_fft 4096 / hop 1024 (508 MB), (N, F, K)'
        roofline['definition'] = ('v2 (rounds 5+): the (N, F, K) kernel the timed step launches, sustained over %d launches since round 6; rounds 1-4 '
                                  'reported the reference-layout (N, K, F) kernel under this key - that series continues as roofline_nkf / frac_nkf' % SUSTAINED_LAUNCHES)
        roofline['frac_config5'] = roofline_config5['frac']
        roofline['frac_nkf'] = roofline_nkf['frac']
        roofline['frac_config5_nkf'] = roofline_config5_nkf['frac']
        roofline_copy = _copy_roofline(device, roofline['bytes_per_launch'])
        roofline['frac_copy'] = roofline_copy['frac']
        roofline['note'] = ('frac: the step\'s STFT kernel (N, F, K) on 1024 clips x 2 s; frac_config5: configs[4] (4096/1024, 32 x 30 s) in the same '
                            'layout (full entry: roofline_config5); frac_nkf / frac_config5_nkf: the same transforms writing the reference\'s (N, K, F) '
                            '(roofline_nkf, roofline_config5_nkf).  Every frac is the mean over 64 back-to-back launches behind >= 150 ms of untimed '
                            'back-to-back launches (SUSTAINED at the running clock: an idle MI355X needs 30-40 ms of work to leave its ~100 MHz idle clock; '
                            'first_launch_us / ramp8_launch_us = the first launches out of idle, best / worst of the 32 beside it; frac_copy = a plain copy of the same bytes under the same timing).  `traffic` fields are RECORDED counter passes (profiles/stft_pmc.json, rocprofv3 '
                            '--pmc in separate runs), not measured in this run')
        roofline_mel = _mel_roofline(device)
        roofline_conv = _conv_roofline(device, N, Fr)
        legs = {}
        if not args.no_legs and world == 1:      # single-GPU legs: each builds a Trainer of its own (a collective set-up under a process group)
            # each leg in a child process under a time limit: a leg that dies or hangs (extra graph branches, a Trainer of its own) costs its
            # own entry, not the line
            legs['config3_step'] = _leg_subprocess('config3')
            legs['config4_step'] = _leg_subprocess('config4')
            legs['dropin_step'] = _leg_subprocess('dropin')
        out = {
            'roofline': roofline, 'roofline_instep': roofline_instep, 'roofline_nkf': roofline_nkf, 'roofline_config5': roofline_config5,
            'roofline_config5_nkf': roofline_config5_nkf, 'roofline_copy': roofline_copy, 'roofline_conv': roofline_conv,
            'roofline_mel': roofline_mel, 'h2d_inclusive': h2d, 'timing': timing,
        }
        out.update(legs)
    return out



def _leg_subprocess(name, limit=180.0):
    import subprocess
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg', name], capture_output=True, text=True, timeout=limit)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
        if r.returncode != 0 or not lines:
            return {'error': 'leg %s: exit code %d: %s' % (name, r.returncode, (r.stderr or '')[-300:])}
        return json.loads(lines[-1])
    except subprocess.TimeoutExpired:
        return {'error': 'leg %s: no result within %.0f s (killed)' % (name, limit)}
    except Exception as e:                                    # noqa: BLE001
        return {'error': 'leg %s: %r' % (name, e)}


def _time_steps(tr, steps, warm):
    """ms/step of a Trainer loop (graph replays), synchronised on both sides; plus the per-step distribution from a HIP event after every step
    (device time between the ends of consecutive steps: no host synchronisation inside the loop)"""
    s = 0
    for _ in range(warm):
        s += 1
        tr.step = s
        tr.train(s)
    torch.cuda.synchronize()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    evs[0].record()
    for i in range(steps):
        s += 1
        tr.step = s
        tr.train(s)
        evs[i + 1].record()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    per = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(steps)])
    dist = {'p50': float(np.percentile(per, 50)), 'p99': float(np.percentile(per, 99)), 'max': float(per.max()), 'min': float(per.min()),
            'steps': int(steps), 'max_over_p50': float(per.max() / np.percentile(per, 50)),
            'note': 'ms between the ends of consecutive steps on the device (one HIP event per step, no host synchronisation in the loop)'}
    return ms, dist


def _config3_build(device):
    """BASELINE configs[2]: 16 segments x 8192 samples (22.05 kHz) per GPU, HiFi-GAN framing mel (1024 / 256 / 80), hifi_gan_v1 generator on
    the channels-last conv kernels (bf16 operands), loss = L1(mel(G(mel(x))), mel(x)), pytorch_sound_amd.optim.Adam, hipGraph replay."""
    from pytorch_sound_amd.models import build_model
    from pytorch_sound_amd.models.vocoders import hifi_gan  # noqa: F401
    from pytorch_sound_amd.interface.hifi_gan import MelSpectrogram
    from pytorch_sound_amd.trainer import Trainer, LogType
    from pytorch_sound_amd import optim as poptim
    from pytorch_sound_amd import kernels as K
    N, T = 16, 8192
    torch.manual_seed(0)
    gen = build_model('hifi_gan_v1').to(device)
    mel = MelSpectrogram().to(device)

    class Step(Trainer):
        def prepare(self, wav):
            with torch.no_grad():
                return wav, mel(wav)

        def forward(self, wav, m, is_logging=False):
            with torch.autocast('cuda', dtype=torch.bfloat16):      # bf16 conv operands: the generator's channels-last kernels (fp32 outside autocast)
                y = self.model(m)
            y = y.float().squeeze(1)
            loss = K.l1_loss(mel(y), m)                 # F.l1_loss as psnd_l1_loss_fwd / _bwd (abs / mean / sign / scale: 5 library launches otherwise)
            self.last_loss = loss.detach()
            return loss, {'loss': (loss, LogType.SCALAR)}

    g = torch.Generator().manual_seed(1 + int(os.environ.get('RANK', '0')))
    pool = [((0.07 * torch.randn(N, T, generator=g)).clamp(-1, 1).to(device),) for _ in range(4)]
    tr = Step(gen, poptim.Adam(gen.parameters(), lr=2e-4, betas=(0.8, 0.99)), pool, pool, max_step=10 ** 9, valid_max_step=1,
              save_interval=10 ** 9, log_interval=10 ** 9, save_dir=tempfile.mkdtemp(prefix='psnd_c3_'), seed=1)
    tr.graph_steps = True
    gen.train()
    # hifi_gan_v1 forward 19.65 GFLOP per 8192-sample segment (conv MACs x 2), x 3 for forward + both gradients
    flops = 19.65e9 * N * 3.0
    meta = {'unit': 'audio-s/s', 'dtype': 'bf16 conv operands under torch.autocast (Generator.precision auto), fp32 accumulate / features / optimizer',
            'workload': 'configs[2] per GPU: hifi_gan_v1 (13.9 M parameters), 16 x 8192-sample segments at 22.05 kHz (F = 32), '
                        'mel 1024/256/80 (HiFi-GAN framing), L1(mel(G(mel x)), mel x), Adam, hipGraph replay; the resblocks of a stage and the upsamplers\' '
                        'parameter-side backward as parallel graph branches (DESIGN 4.4)',
            'model_params': sum(p.numel() for p in gen.parameters()), 'flops_per_step': flops,
            'flops_note': 'SURVEY 8(d): 19.65 GFLOP forward per segment x 16 segments x 3 (forward + input + weight gradients); mel / loss / Adam not counted'}
    return tr, N * T / SR, meta


def _config4_build(device, T=1292):
    """BASELINE configs[3] block: 1x1 projection of an 80-mel input -> PositionalEncoding -> MultiHeadAttention(256, 4) ->
    PointwiseFeedForward -> 1x1, batch 32 per GPU at the 15-s bucket (1292 frames), padding mask (lengths 0.8 .. 1.0 of the bucket),
    masked L1 to the input, Adam, bf16 operands under autocast (fp32 scores / statistics), hipGraph replay."""
    from pytorch_sound_amd.models import modules as M
    from pytorch_sound_amd.trainer import Trainer, LogType
    from pytorch_sound_amd import optim as poptim
    from pytorch_sound_amd import kernels as K
    C, H, N = 256, 4, 32

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.inp = torch.nn.Conv1d(80, C, 1)
            self.pe = M.PositionalEncoding(C, 2048)
            self.mha = M.MultiHeadAttention(C, H, 0.0)
            self.ffn = M.PointwiseFeedForward(C, 0.0)
            self.out = torch.nn.Conv1d(C, 80, 1)

        def forward(self, mel_, pad_mask):
            x = self.pe(M._conv1x1(self.inp, mel_))
            x, _ = self.mha(x, pad_mask)
            return M._conv1x1(self.out, self.ffn(x))

    torch.manual_seed(0)
    net = Net().to(device)
    net.mha.return_att = False

    class Step(Trainer):
        def forward(self, mel_, valid, pad, is_logging=False):
            with torch.autocast('cuda', dtype=torch.bfloat16):
                y = self.model(mel_, pad)
            loss = K.masked_l1_loss(y.float(), mel_, valid)
            self.last_loss = loss.detach()
            return loss, {'loss': (loss, LogType.SCALAR)}

    g = torch.Generator().manual_seed(2 + int(os.environ.get('RANK', '0')))
    lens = torch.linspace(0.8 * T, T, N).long()
    valid = (torch.arange(T)[None, :] < lens[:, None]).float().to(device)
    pad = valid < 0.5                                    # the padding mask comes with the batch (the collate function knows the lengths)
    pool = [(torch.randn(N, 80, T, generator=g).to(device), valid, pad) for _ in range(3)]
    tr = Step(net, poptim.Adam(net.parameters(), lr=1e-4), pool, pool, max_step=10 ** 9, valid_max_step=1, save_interval=10 ** 9,
              log_interval=10 ** 9, save_dir=tempfile.mkdtemp(prefix='psnd_c4_'), seed=1)
    tr.graph_steps = True
    net.train()
    # transformer block 2 * 12 C^2 + 4 C T flop per frame forward, + the two 1x1 projections 2 * 2 * 80 * C; x 3 for the backward
    flops = (24.0 * C * C + 4.0 * C * T + 4.0 * 80 * C) * N * T * 3.0
    meta = {'unit': 'audio-s/s (unpadded)', 'dtype': 'bf16 operands under autocast, fp32 scores / statistics / accumulation',
            'workload': 'configs[3] block per GPU: 80-mel -> 1x1 -> PositionalEncoding -> MultiHeadAttention(256, 4) -> '
                        'PointwiseFeedForward -> 1x1, batch 32 x %d frames (15-s bucket, lengths 0.8-1.0 of it, padding mask), masked L1, '
                        'Adam, hipGraph replay; the 1x1 projections\' parameter-side backward as a parallel graph branch (DESIGN 4.4)' % T,
            'model_params': sum(p.numel() for p in net.parameters()), 'flops_per_step': flops,
            'flops_note': 'SURVEY 8(d): (24 C^2 + 4 C T + 4 * 80 C) flop per frame forward (C = 256, T = 1292) x 32 x 1292 frames x 3 (forward + backward)'}
    return tr, float(lens.sum()) * HOP / SR, meta


def _leg(device, build, steps, warm):
    tr, audio_s, meta = build(device)
    ms, dist = _time_steps(tr, steps, warm)
    out = {'ms_per_step': ms, 'value': audio_s / (ms * 1e-3), 'steps': steps, 'warmup': warm, 'n_gpus': 1, 'step_ms': dist,
           'mfma_frac': meta['flops_per_step'] / (ms * 1e-3) / MFMA_BF16_PEAK, 'mfma_peak': 'dense bf16 MFMA 2.5 PFLOP/s'}
    out.update(meta)
    return out


def _config3_leg(device, steps=200, warm=10):
    return _leg(device, _config3_build, steps, warm)


def _config4_leg(device, steps=200, warm=6):
    return _leg(device, _config4_build, steps, warm)


def _dropin_leg(device, steps=60, warm=8):
    """configs[1] written ONLY with the reference's API names, the way a user of pytorch_sound writes a step (trainer.py:58-73: override
    Trainer.forward): STFT.transform on the waveforms inside forward (magnitude AND phase, as the reference computes them),
    build_model('conv_separator_voicebank') under autocast, LogMelSpectrogram for the target, the mel of the estimate as torch ops on the
    module's `mel_filter` buffer, F.l1_loss.  No prepare(), no library-only layout / fused-loss entry points.  Eager and with graph_steps."""
    from pytorch_sound.models import build_model
    from pytorch_sound.models.transforms import LogMelSpectrogram
    from pytorch_sound.trainer import Trainer, LogType
    from pytorch_sound_amd.models import separator  # noqa: F401  (registers conv_separator)
    from pytorch_sound_amd import optim as poptim
    T, N = int(SR * CLIP_SECONDS), BATCH_PER_GPU
    fe = LogMelSpectrogram(SR, N_MEL, N_FFT, N_FFT, HOP, -50, 30, FMIN, FMAX).to(device)

    class Step(Trainer):
        def forward(self, both, is_logging=False):
            n = both.shape[0] // 2
            noisy, clean = both[:n], both[n:]
            with torch.no_grad():
                mag_ref, _ = fe.stft.transform(clean)
                mel_ref = fe(clean)
            mag_mix, _ = fe.stft.transform(noisy)
            with torch.autocast('cuda', dtype=torch.bfloat16):
                est = self.model(mag_mix)
            est = est.float()
            mel_est = torch.log(torch.matmul(fe.mel_filter, est) + 1e-6).clamp(fe.min_db, fe.max_db)
            loss = F.l1_loss(est, mag_ref) + 0.5 * F.l1_loss(mel_est, mel_ref)
            return loss, {'loss': (loss, LogType.SCALAR)}

    res = {}
    for mode in ('default', 'eager', 'graph_steps'):
        torch.manual_seed(1234)
        model = build_model('conv_separator_voicebank').to(device)
        pool = [synth_batch(1234 + 1000 * i, N, T, device) for i in range(4)]
        # the optimizer as the reference's recipes build it: a stock torch.optim.Adam (Trainer adopts it: pytorch_sound_amd.optim.Adam's launch)
        tr = Step(model, torch.optim.Adam(model.parameters(), lr=2e-4, betas=(0.8, 0.99)), pool, pool, max_step=10 ** 9, valid_max_step=1,
                  save_interval=10 ** 9, log_interval=10 ** 9, save_dir=tempfile.mkdtemp(prefix='psnd_dropin_'), seed=1234)
        if mode != 'default':                              # 'default': Trainer.graph_steps = 'auto' - nothing set by the caller
            tr.graph_steps = mode == 'graph_steps'
        model.train()
        try:
            ms, dist = _time_steps(tr, steps, warm + tr.graph_warmup + 1)
            res[mode] = {'ms_per_step': ms, 'value': N * CLIP_SECONDS / (ms * 1e-3), 'step_ms': dist,
                         'captured': bool(any('graph' in v for v in getattr(tr, '_graphs', {}).values())),
                         'optimizer': type(tr.optimizer).__module__ + '.' + type(tr.optimizer).__name__}
        except Exception as e:                                  # noqa: BLE001 - a mode that cannot run is reported, not fatal
            res[mode] = {'error': repr(e)[:300]}
    res.update({'unit': 'audio-s/s', 'n_gpus': 1, 'steps': steps, 'dtype': 'bf16 autocast around the model, fp32 features / loss',
                'workload': 'configs[1] (32 x 2 s, conv_separator_voicebank, Adam) with the step written against the reference\'s API only: '
                            'Trainer.forward override, STFT.transform (magnitude and phase) x 2 + LogMelSpectrogram inside forward, torch.matmul / '
                            'log / clamp on `mel_filter` for the mel of the estimate, F.l1_loss x 2 - what a user gets who switches the import and '
                            'changes nothing else = the `default` entry (Trainer.graph_steps = \'auto\' captures a step whose forward() is free of host-side randomness / step-count reads, a stock torch.optim.Adam is adopted; `eager` / `graph_steps`: the switch set by hand) (round 6: the model hands out its estimate as a deferred tensor, pytorch_sound_amd/deferred.py - those torch '
                            'ops are recorded and resolve to the fused loss node, and STFT.transform hands out its magnitude bin-fastest (N, F, K) as a deferred tensor standing for (N, K, F), the phase on first use; gc.freeze() after the first steps ends the 50-120 ms cyclic-GC steps of the '
                            'eager loop); the headline `value` is the same step on the library\'s prepare() / (N, F, K) / fused-loss API'})
    return res


def _flush_c_stdio():
    """RCCL prints its version banner through C stdio, which is block-buffered when stdout is a pipe: left alone it comes out when the process
    exits - BEHIND the JSON line, on every rank.  Flushed here (right behind the communicator's first collective, and again in front of the
    line) so that the JSON line is the last thing rank 0 writes."""
    import ctypes
    try:
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)
    except Exception:      # noqa: BLE001
        pass


def _emit_line(out):
    """barrier, tear the process group down, flush what C code buffered, then the one JSON line (rank 0) as the last write"""
    _flush_c_stdio()                                 # every rank: its buffered banner out BEFORE the barrier below ...
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.barrier()                  # ... so that nothing of another rank can land behind rank 0's line
        torch.distributed.destroy_process_group()
    _flush_c_stdio()
    if out is not None:
        print(json.dumps(out), flush=True)


def _dist_setup(args):
    from pytorch_sound_amd import distributed as pdist
    if args.force_ddp and int(os.environ.get('WORLD_SIZE', '1')) <= 1:
        # one-rank RCCL process group: the whole data-parallel step (flat buckets, captured all-reduce) on one GPU
        os.environ.update(PSND_DDP_FORCE='1', MASTER_ADDR='127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29519')
        torch.cuda.set_device(0)
        torch.distributed.init_process_group('nccl', rank=0, world_size=1)
    distributed = pdist.init_from_env('nccl')
    rank, world = pdist.rank(), pdist.world_size()
    if world != args.gpus:
        raise SystemExit('--gpus %d but WORLD_SIZE=%d: launch with torch.distributed.run' % (args.gpus, world))
    local = 0 if os.environ.get('PSND_DIST_SHARE_GPU') == '1' else int(os.environ.get('LOCAL_RANK', '0'))
    torch.cuda.set_device(local)
    if distributed or (torch.distributed.is_available() and torch.distributed.is_initialized()):
        torch.distributed.barrier()              # the communicator exists (and has printed its banner) on every rank
        _flush_c_stdio()
    return distributed, rank, world, torch.device('cuda', local)


def config_bench(args):
    """--config 3 | 4 | 5 (with --gpus N under torch.distributed.run): the data-parallel runs of BASELINE configs[2] / [3] / [4] under the same
    contract as the headline line - W warm-up steps, K timed steps between barriers, the maximum over the ranks, whole-job audio-s/s.
    Configs 3 and 4: one process per GPU, flat gradient buckets all-reduced over RCCL (distributed.FlatGradReducer, captured into the step
    graph); config 5 is feature extraction only (32 x 30 s clips per GPU through psnd_stft_mag_nfk): clips shard, no collective."""
    distributed, rank, world, device = _dist_setup(args)

    def barrier():
        torch.cuda.synchronize()
        if distributed:
            torch.distributed.barrier()
            torch.cuda.synchronize()

    if args.config == 5:
        from pytorch_sound_amd import kernels as K
        n_fft, hop, clips, T = 4096, 1024, 32, int(44100 * 30.0)
        g = torch.Generator().manual_seed(5 + rank)
        wav = (0.07 * torch.randn(clips, T, generator=g)).to(device)
        plan = K.stft_plan(n_fft, _hann(n_fft)).to(device)
        mag = torch.empty(clips, K.frame_count(T, n_fft, hop), n_fft // 2 + 1, device=device)

        def one_step():
            K.stft_mag_nfk(wav, n_fft, hop, plan, out=mag)
        audio_s, meta = clips * 30.0, {'unit': 'audio-s/s', 'dtype': 'f32', 'model_params': 0,
                                       'workload': 'configs[4] per GPU: 32 clips x 30 s at 44.1 kHz, STFT 4096 / 1024 magnitude, (N, F, K) output '
                                                   '(508 MB of algorithmic traffic per step): feature extraction only, clips shard across GPUs, no collective'}
        bytes_step = 4.0 * clips * T + 4.0 * mag.numel()
    else:
        tr, audio_s, meta = (_config3_build if args.config == 3 else _config4_build)(device)
        st = [0]

        def one_step():
            st[0] += 1
            tr.step = st[0]
            tr.train(st[0])
        bytes_step = None
    for _ in range(args.settle + args.warmup + (8 if args.config != 5 else 0)):
        one_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        one_step()
    barrier()
    dt = time.perf_counter() - t0
    if distributed:
        tdt = torch.tensor([dt], device=device, dtype=torch.float64)
        torch.distributed.all_reduce(tdt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tdt.item())
    if args.dump_outputs and rank == 0:
        bench_outputs(args.dump_outputs, {'mag': mag} if args.config == 5 else _trainer_outputs(tr))
    if rank != 0:
        return None
    red = getattr(tr, '_reducer', None) if args.config != 5 else None
    out = {'metric': 'audio-sec/s STFT+mel+fwd/bwd' if args.config != 5 else 'audio-sec/s STFT (feature extraction only)',
           'reducer': None if red is None else {'active': bool(red.active), 'buckets': len(red.buckets),
                                                'graph_modes': [v.get('ddp') for v in getattr(tr, '_graphs', {}).values() if 'graph' in v]},
           'value': world * audio_s * args.steps / dt, 'unit': 'audio-s/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
           'settle': args.settle, 'ms_per_step': dt / args.steps * 1e3, 'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
           'dtype': 'bf16' if args.config != 5 else 'f32', 'data': 'synthetic',
           'config': {'workload': meta['workload'], 'parallelism': 'dp%d' % world, 'model_params': meta['model_params'], 'baseline_config': args.config - 1}}
    if args.config == 5:
        out['roofline'] = {'bound': 'hbm', 'achieved': bytes_step * args.steps / dt / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s',
                           'frac': bytes_step * args.steps / dt / HBM_PEAK, 'traffic': None, 'kernel': 'stft_fwd_n4096r_kernel',
                           'note': 'per GPU, host-timed over the K launches of the contract region (includes the launch gaps)'}
    else:
        out['mfma_frac'] = meta['flops_per_step'] * world * args.steps / dt / (world * MFMA_BF16_PEAK)
    return out


SUSTAINED_LAUNCHES = 64      # back-to-back launches behind every roofline figure (a burst of 8 flattered config 5 by 20 %)
SUSTAINED_WARM_S = 0.15      # untimed back-to-back launches in front of them.  An idle MI355X sits at sclk ~100 MHz and takes ~30-40 ms of
                             # continuous work to reach its running clock (tools/r06/series.py, profiles/r06_launch_series.txt: the n = 1024 kernel
                             # reads 150-165 us for its first 48 launches out of idle, 111-113 us from launch ~250 on and stays there for 1024
                             # launches; a plain copy of the same bytes 102-103 us throughout) - 8 untimed launches (round 5 / the first round-6
                             # line) timed that RAMP, not the kernel


def _time_launches(launch, n=SUSTAINED_LAUNCHES, warm_s=SUSTAINED_WARM_S):
    """HIP events around each of `n` back-to-back launches on the current stream, behind >= `warm_s` seconds of untimed back-to-back launches (the
    clock ramp out of idle): the SUSTAINED mean over the n (what the `frac` fields are computed from), the first launch of the whole run (cold:
    clocks and caches), the best one, and the mean of the first 8 launches out of idle (`ramp8`: what a short burst reads), in seconds"""
    torch.cuda.synchronize()
    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    head = []
    for _ in range(8):                                   # the first launches out of idle, timed for the record
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        head.append((e0, e1))
    warm_launches, t0 = 8, time.perf_counter()
    while time.perf_counter() - t0 < warm_s:
        for _ in range(64):
            launch()
        warm_launches += 64
        torch.cuda.synchronize()
    evs = []
    for _ in range(64):                                  # (no gap between the last warm chunk and the timed launches)
        launch()
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    hs = [a.elapsed_time(b) * 1e-3 for a, b in head]
    ts = [a.elapsed_time(b) * 1e-3 for a, b in evs]
    return {'t': float(np.mean(ts)), 'first': hs[0], 'best': float(np.min(ts)), 'worst': float(np.max(ts)), 'ramp8': float(np.mean(hs)), 'n': n,
            'warm_launches': warm_launches + 64}


def _launch_fields(m):
    return {'launch_us': m['t'] * 1e6, 'launches_timed': m['n'], 'untimed_launches_before': m['warm_launches'], 'first_launch_us': m['first'] * 1e6,
            'best_launch_us': m['best'] * 1e6, 'worst_launch_us': m['worst'] * 1e6, 'ramp8_launch_us': m['ramp8'] * 1e6}


def _copy_roofline(device, nbytes):
    """a plain device copy moving the same number of bytes as the judged STFT launch (nbytes / 2 read + nbytes / 2 written): what this box's HBM
    delivers to the simplest kernel there is, under the same timing"""
    a = torch.empty(nbytes // 8, device=device)
    b = torch.empty_like(a)
    m = _time_launches(lambda: b.copy_(a))
    return {'bound': 'hbm', 'kernel': 'torch copy_ (fp32, %d MB read + %d MB written)' % (nbytes // 2e6, nbytes // 2e6), 'achieved': nbytes / m['t'] / 1e9,
            'peak': HBM_PEAK / 1e9, 'unit': 'GB/s', 'frac': nbytes / m['t'] / HBM_PEAK, 'bytes_per_launch': nbytes, **_launch_fields(m)}


def _nfk_roofline(device, n_fft, hop, clips, T, label):
    """psnd_stft_mag_nfk (magnitude with the bin axis fastest, (N, F, K)): the same algorithmic bytes as psnd_stft_fwd, HIP events around every launch"""
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    wav = torch.randn(clips, T, device=device) * 0.07
    plan = K.stft_plan(n_fft, _hann(n_fft)).to(device)
    Kb, Fr = n_fft // 2 + 1, K.frame_count(T, n_fft, hop)
    mag = torch.empty(clips, Fr, Kb, device=device)
    m = _time_launches(lambda: check(lib().psnd_stft_mag_nfk(ptr(wav), clips, T, n_fft, hop, 0, ptr(plan), 0.0, ptr(mag), stream_ptr(device)),
                                     'psnd_stft_mag_nfk'))
    t = m['t']
    b = 4 * clips * T + 4 * clips * Kb * Fr
    return {'bound': 'hbm', 'kernel': label, 'achieved': b / t / 1e9, 'peak': HBM_PEAK / 1e9, 'unit': 'GB/s', 'frac': b / t / HBM_PEAK,
            'traffic': _pmc_traffic('nfk%d' % n_fft), 'bytes_per_launch': b, **_launch_fields(m),
            'traffic_source': _pmc_traffic('nfk%d' % n_fft, 'source'),
            'layout': '(N, F, K): bin axis fastest - what the consumers inside the library (mel kernel, channels-last conv stack, spectral losses) take'}


def _mel_roofline(device, clips=1024, Fr=173, Kb=513, M=80):
    """SURVEY 8(d) mel stage unfused: psnd_mel_fwd on (clips, K, F) magnitudes: 4NKF + 4NMF bytes per launch"""
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd.utils.mel import mel_filterbank
    plan = K.mel_plan(mel_filterbank(SR, N_FFT, M, FMIN, FMAX)).to(device)
    mag = torch.rand(clips, Kb, Fr, device=device)
    out = torch.empty(clips, M, Fr, device=device)
    m = _time_launches(lambda: K.mel_forward(mag, plan, M, K.LOG_E, 1e-6, None, -11.5, 6.9, out=out))
    t = m['t']
    b = 4 * clips * Kb * Fr + 4 * clips * M * Fr
    return {'bound': 'hbm', 'kernel': 'mel_fwd_once_kernel<5> (band-sparse fp32 MFMA 16x16x4, a wave owns all five mel tiles of its 64 frames: every magnitude read once; (N,K,F) -> log-mel (N,M,F))', 'achieved': b / t / 1e9,
            'peak': HBM_PEAK / 1e9, 'unit': 'GB/s', 'frac': b / t / HBM_PEAK, 'traffic': _pmc_traffic('mel'), 'traffic_source': _pmc_traffic('mel', 'source'),
            'bytes_per_launch': b, **_launch_fields(m), 'flops_per_launch': 2.0 * M * Kb * clips * Fr,
            'workload': '%d clips x 2 s: %d x %d x %d magnitudes -> %d mel bands (%.0f MB)' % (clips, clips, Kb, Fr, M, b / 1e6)}


def _config5_roofline(device, n_fft=4096, hop=1024, clips=32, seconds=30.0, sr=44100):
    """BASELINE config 5 (Maestro-like 44.1 kHz music, 4096-pt STFT, 30 s clips): psnd_stft_fwd magnitude on 32 clips
    (169 MB in + 339 MB out = 508 MB), HIP events around every launch"""
    from pytorch_sound_amd import kernels as K
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    T = int(sr * seconds)
    wav = torch.randn(clips, T, device=device) * 0.07
    plan = K.stft_plan(n_fft, _hann(n_fft)).to(device)
    Kb, Fr = n_fft // 2 + 1, K.frame_count(T, n_fft, hop)
    mag = torch.empty(clips, Kb, Fr, device=device)
    m = _time_launches(lambda: check(lib().psnd_stft_fwd(ptr(wav), clips, T, n_fft, hop, 0, ptr(plan), 0.0, ptr(mag), None, None, None,
                                                         stream_ptr(device)), 'psnd_stft_fwd'))
    t = m['t']
    b = 4 * clips * T + 4 * clips * Kb * Fr
    kern = ('stft_fwd_n4096w_kernel (one wave per frame, 16 frames per workgroup, 64-byte store runs)' if clips * ((Fr + 15) // 16) >= 2048
            else 'stft_fwd_n4096b_kernel (4 frames per workgroup)')
    return {'bound': 'hbm', 'kernel': kern + ': wav -> magnitude, 4096/1024', 'achieved': b / t / 1e9,
            'peak': HBM_PEAK / 1e9, 'unit': 'GB/s', 'frac': b / t / HBM_PEAK, 'traffic': _pmc_traffic('n4096'),
            'traffic_source': _pmc_traffic('n4096', 'source'), 'bytes_per_launch': b,
            **_launch_fields(m),
            'workload': 'configs[4]: %d clips x %.0f s at %d Hz, n_fft %d / hop %d (%.0f MB)' % (clips, seconds, sr, n_fft, hop, b / 1e6)}


def _conv_roofline(device, N, Fr, C=256, k=3, dil=1, iters=50):
    """the kernels that take most of the step (profiles/): one ResBlock conv of the config-2 model (C -> C channels, k = 3, on
    N x Fr frames) forward (conv_cl_kernel; two chained convs of a residual pair: conv_pair_kernel) and backward (conv_bwd_pair_kernel:
    input gradient + weight-gradient slabs), launched back to back and timed with HIP events; flops = 2 N Fr C C k per GEMM, against the dense bf16 MFMA peak."""
    from pytorch_sound_amd import cl
    from pytorch_sound_amd._lib import lib, ptr, stream_ptr, check
    HP = 8
    shape = cl.CLShape(N, Fr, HP)
    Lp = shape.Lp
    x = torch.randn(N, Lp, C, device=device).to(torch.bfloat16)
    g1 = torch.randn(N, Lp, C, device=device).to(torch.bfloat16)
    g2 = torch.randn(N, Lp, C, device=device).to(torch.bfloat16)
    w = (torch.randn(k, C, C, device=device) * 0.05).to(torch.bfloat16)
    bias = torch.zeros(C, device=device)
    out = torch.empty_like(x)
    act = torch.empty_like(x)
    gx = torch.empty_like(x)
    S = lib().psnd_conv1d_cl_wgrad_splits(N, Lp, C, C, k)
    gw = torch.empty(S, k, C, C, device=device)
    gbp = torch.empty(S, C, device=device)
    st = stream_ptr(device)

    def fwd():
        check(lib().psnd_conv1d_cl(ptr(x), None, None, 0.0, ptr(w), ptr(bias), None, None, N, Lp, Fr, HP, C, C, k, -dil, dil, 0.1, 1.0,
                                   ptr(out), ptr(act), None, st), 'psnd_conv1d_cl')

    def bwd():
        # the launch as it runs inside a residual block: one plain incoming gradient, epilogue forms the next conv's
        check(lib().psnd_conv1d_cl_bwd(ptr(g1), None, None, 0.1, ptr(w), ptr(x), N, Lp, Fr, HP, C, C, k, dil, dil, ptr(gx), None,
                                       ptr(act), 0.1, ptr(g1), ptr(gw), ptr(gbp), st), 'psnd_conv1d_cl_bwd')

    w2 = (torch.randn(k, C, C, device=device) * 0.05).to(torch.bfloat16)
    mid = torch.empty_like(x)

    def fwd_pair():
        # conv(d = 3) -> leaky -> conv(1) -> + x of a residual pair as ONE launch (psnd_conv1d_cl_pair, csrc/psnd_conv_pair.hip)
        check(lib().psnd_conv1d_cl_pair(ptr(x), ptr(w), ptr(bias), None, 1.0, 0.1, ptr(mid), ptr(w2), ptr(bias), None, 1.0, ptr(x), N, Lp, Fr,
                                        HP, C, k, -3, 3, -1, 1, 0.1, ptr(out), ptr(act), st), 'psnd_conv1d_cl_pair')

    S2 = lib().psnd_conv1d_cl_pair_bwd_splits(N, Lp, C, k)
    gwa, gba = torch.empty(S2, k, C, C, device=device), torch.empty(S2, C, device=device)
    gwb, gbb = torch.empty(S2, k, C, C, device=device), torch.empty(S2, C, device=device)
    gmid = torch.empty_like(x)

    def bwd_pair2():
        # the backward of a whole residual pair as it runs in the step (psnd_conv1d_cl_pair_bwd): both input gradients chained on chip +
        # the weight gradients of the pair's second conv and of the previous pair's first conv: four GEMMs
        check(lib().psnd_conv1d_cl_pair_bwd(ptr(g1), ptr(w2), ptr(act), 0.1, ptr(gmid), ptr(w), ptr(x), 0.1, ptr(g1), N, Lp, Fr, HP, C, k, 1, 1, 3, 3,
                                            ptr(gx), ptr(act), ptr(gwa), ptr(gba), ptr(g2), ptr(x), -3, 3, ptr(gwb), ptr(gbb), st),
              'psnd_conv1d_cl_pair_bwd')

    # ---- the launches the step runs since round 3 (cl.py: _chain_pairs, batched backward): a ResBlock1 (three residual pairs, dilations
    # 1 / 3 / 5) forward as ONE launch, its input gradients as ONE masked launch, the weight gradients of all 24 body convs as ONE launch
    import ctypes
    from pytorch_sound_amd import _lib
    ws = [(torch.randn(k, C, C, device=device) * 0.05).to(torch.bfloat16) for _ in range(6)]
    outs = [[torch.empty_like(x) for _ in range(3)] for _ in range(3)]

    def chain_desc(masked):
        arr = (_lib.ChainPair * 3)()
        for i, (d, dd) in enumerate(zip(arr, (1, 3, 5))):
            d.W1, d.bias1, d.act1_slope, d.mid_out = ws[2 * i].data_ptr(), None if masked else bias.data_ptr(), 1.0 if masked else 0.1, outs[i][0].data_ptr()
            d.W2, d.bias2, d.off1, d.dstep1, d.off2, d.dstep2 = ws[2 * i + 1].data_ptr(), None if masked else bias.data_ptr(), -dd, dd, -1, 1
            d.act2_slope, d.out_raw, d.out_act = (1.0 if masked else 0.1), outs[i][1].data_ptr(), None if masked else outs[i][2].data_ptr()
            if masked:
                d.M1, d.M2, d.m1_slope, d.m2_slope = act.data_ptr(), x.data_ptr(), 0.1, 0.1
        return arr
    arr_f, arr_b = chain_desc(False), chain_desc(True)

    def fwd_chain():
        check(lib().psnd_conv1d_cl_chain(ptr(x), ptr(g2), ctypes.addressof(arr_f), 3, N, Lp, Fr, HP, C, k, st), 'psnd_conv1d_cl_chain')

    def bwd_chain():
        check(lib().psnd_conv1d_cl_chain(ptr(g1), ptr(g1), ctypes.addressof(arr_b), 3, N, Lp, Fr, HP, C, k, st), 'psnd_conv1d_cl_chain')

    NW = 24
    Sm = lib().psnd_conv1d_cl_wgrad_multi_splits(N, Lp, C, C, k, NW)
    gs = [torch.randn(N, Lp, C, device=device).to(torch.bfloat16) for _ in range(NW)]
    xs = [torch.randn(N, Lp, C, device=device).to(torch.bfloat16) for _ in range(NW)]
    gwm = [torch.empty(Sm, k, C, C, device=device) for _ in range(NW)]
    gbm = [torch.empty(Sm, C, device=device) for _ in range(NW)]
    wd = (_lib.WgradDesc * NW)()
    for i, d in enumerate(wd):
        dd = (1, 1, 3, 1, 5, 1)[i % 6]
        d.g, d.xa, d.gw_part, d.gbias_part, d.off0, d.dstep = gs[i].data_ptr(), xs[i].data_ptr(), gwm[i].data_ptr(), gbm[i].data_ptr(), -dd, dd
        d.Ca, d.Cb, d.k, d.splits = C, C, k, Sm

    def wgrad_multi():
        check(lib().psnd_conv1d_cl_wgrad_multi(ctypes.addressof(wd), NW, N, Lp, st), 'psnd_conv1d_cl_wgrad_multi')

    res = {}
    for name, f, gemms in (('forward', fwd, 1), ('forward_pair', fwd_pair, 2), ('backward_pair', bwd, 2), ('backward_pair2', bwd_pair2, 4),
                           ('forward_chain', fwd_chain, 6), ('input_gradient_chain', bwd_chain, 6), ('weight_gradients_24', wgrad_multi, NW)):
        for _ in range(5):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            f()
        e1.record()
        torch.cuda.synchronize()
        t = e0.elapsed_time(e1) / iters * 1e-3
        flops = gemms * 2.0 * N * Fr * C * C * k          # algorithmic: the rims a chain launch recomputes are not counted
        res[name] = {'launch_us': t * 1e6, 'flops_per_launch': flops, 'achieved': flops / t / 1e12, 'frac': flops / t / MFMA_BF16_PEAK}
    # the body's 24 convs per step: 4 forward chains + 4 input-gradient chains + one weight-gradient launch = 72 GEMMs
    t_body = 4 * res['forward_chain']['launch_us'] + 4 * res['input_gradient_chain']['launch_us'] + res['weight_gradients_24']['launch_us']
    f_body = 72 * 2.0 * N * Fr * C * C * k
    return {'bound': 'mfma', 'unit': 'TFLOP/s', 'peak': MFMA_BF16_PEAK / 1e12, 'dtype': 'bf16 operands, fp32 accumulate',
            'kernel': 'the conv body of the config-2 model as the step runs it (cl.py): conv_chain_kernel<..., false> (a ResBlock1 = three residual '
                      'pairs forward in one launch: forward_chain), conv_chain_kernel<..., true> (their input gradients: input_gradient_chain), '
                      'conv_wgrad_multi_kernel (the weight gradients of all 24 body convs in one launch: weight_gradients_24) - 2.2 GFLOP per '
                      '256->256 k=3 GEMM on 3 MB of activations; achieved / frac = the 72 GEMMs of the body over 4 + 4 + 1 such launches back '
                      'to back; the round-2 launches (forward_pair, backward_pair2, ...) are timed beside them.  DESIGN.md 4.4',
            'achieved': f_body / (t_body * 1e-6) / 1e12, 'frac': f_body / (t_body * 1e-6) / MFMA_BF16_PEAK, 'body_us': t_body, **res}


def _event_pair_overhead(device, n=40):
    """median elapsed time of an EMPTY HIP event pair on a stream kept busy by a small kernel in front of it"""
    x = torch.zeros(1 << 22, device=device)
    pairs = []
    for _ in range(n):
        x.add_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in pairs])) * 1e-3


def _hann(n):
    m = np.arange(n)
    return (0.5 - 0.5 * np.cos(2 * np.pi * m / n)).astype(np.float32)


def _pmc_traffic(which, field='hbm_bytes_per_launch'):
    """HBM bytes per launch (FETCH_SIZE x 2 + WRITE_SIZE, MI355X_MICROARCH.md corrections) of the launch the roofline entry times,
    from the committed PMC pass: profiles/stft_pmc.json, written by tools/pmc_to_json.py from separate `rocprofv3 --pmc` runs of
    tools/run_stft_only.py (counters cannot be read inside an un-profiled run).  which: 'n1024' | 'n4096'."""
    p = os.path.join(ROOT, 'profiles', 'stft_pmc.json')
    try:
        return json.load(open(p))[which].get(field)
    except Exception:
        return None


def cpu_baseline(seconds, frontend='port'):
    """reference CPU path on the host cores: same step, fp32, 4 x 2 s clips.  frontend 'port': the reference's dense-DFT conv1d STFT
    (STFT.transform, the class LogMelSpectrogram uses); 'torch_stft': its torch.stft wrapper (STFTTorchAudio) - BASELINE.md asks for
    both."""
    # probe on the MI355X host (256 logical CPUs): this step scales to ~16-32 threads and collapses
    # beyond 64 (oversubscribed small convs), so the baseline uses min(32, cores) threads
    cores = min(32, os.cpu_count() or 1)
    torch.set_num_threads(cores)
    dev = torch.device('cpu')
    Trainer, model = build_step(dev, amp=False, cpu_frontend=frontend)
    Trainer.move_batches_to_gpu = False              # this leg stays on the host (Trainer would .cuda() every batch)
    Ncpu, T = 4, int(SR * CLIP_SECONDS)
    pool = [synth_batch(4321 + i, Ncpu, T, dev) for i in range(2)]
    opt = torch.optim.Adam(model.parameters(), lr=2e-4, betas=(0.8, 0.99))
    huge = 10 ** 9
    tr = Trainer(model, opt, pool, pool, max_step=huge, valid_max_step=1, save_interval=huge, log_interval=huge,
                 save_dir=tempfile.mkdtemp(prefix='psnd_cpu_'), save_prefix='cpu', seed=1234)
    model.train()
    tr.step = 1
    tr.train(1)                                      # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        n += 1
        tr.step = n + 1
        tr.train(n + 1)
        el = time.perf_counter() - t0
        if el >= seconds or n >= 200:
            break
    # the feature path alone (wav -> magnitude -> log-mel of 2 x 4 clips, as prepare() runs it), same threads
    both = pool[0][0]
    tr.prepare(both)
    m, t1 = 0, time.perf_counter()
    while True:
        m += 1
        tr.prepare(both)
        ef = time.perf_counter() - t1
        if ef >= min(2.0, seconds / 4) or m >= 200:
            break
    feat = {'port': "oracle/torch_ref.py RefSTFT (the reference's dense-DFT conv1d STFT, transforms.py:53-69) + mel",
            'torch_stft': "oracle/torch_ref.py RefSTFTTorch (the reference's torch.stft wrapper, transforms.py:297-311) + mel"}[frontend]
    return {'value': n * Ncpu * CLIP_SECONDS / el, 'unit': 'audio-s/s', 'cores': cores, 'cpu_count': os.cpu_count(), 'kind': 'port',
            'frontend': frontend, 'features_only_audio_s_per_s': m * 2 * Ncpu * CLIP_SECONDS / ef,
            'threads_note': 'torch.set_num_threads(min(32, cpu_count)): this step scales to ~16-32 threads and collapses beyond 64',
            'sample': '%d steps of batch 4 x 2 s clips (configs[0] batch), same model/loss/Adam in fp32, '
                      'feature path = %s; %.1f s' % (n, feat, el)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=30, help='timed steps (ms_per_step = their time / steps)')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--full', action='store_true',
                    help='besides the headline: timing spread, host-memory batches, rooflines, config-3 / config-4 / drop-in legs, CPU baselines')
    ap.add_argument('--dump-outputs', metavar='DIR',
                    help='write what the last timed step computed (loss, parameters, gradients; config 5: magnitudes) as DIR/<name>.npy, float32')
    ap.add_argument('--pool', type=int, default=8, help='distinct synthetic batches resident in HBM')
    ap.add_argument('--settle', type=int, default=40, help='untimed set-up steps in front of the W warm-up steps (clock ramp)')
    ap.add_argument('--cpu-seconds', type=float, default=20.0, help='(--full) CPU baseline budget (60 %% dense-DFT port, 40 %% torch.stft variant)')
    ap.add_argument('--no-graph', action='store_true', help='enqueue every kernel of the step eagerly (no hipGraph replay)')
    ap.add_argument('--prefetch', action='store_true', help='stage the next batch (copy + feature extraction) on a side stream')
    ap.add_argument('--unfused-loss', action='store_true', help='the loss as separate nodes (mask head, mel, two L1 terms) instead of the fused one')
    ap.add_argument('--no-legs', action='store_true', help='(--full) skip the bounded config-3 / config-4 step legs (config3_step, config4_step)')
    ap.add_argument('--force-ddp', action='store_true', help='single GPU with a one-rank RCCL group: the data-parallel reducer path on one device')
    ap.add_argument('--no-handover', action='store_true', help='(with a reducer) gradients reach the buckets through autograd hooks only (round 3)')
    ap.add_argument('--overlap-prepare', action='store_true', help="the next batch's feature extraction behind this step's backward on a side stream (Trainer.overlap_prepare)")
    ap.add_argument('--layout', choices=('nfk', 'nkf'), default='nfk',
                    help="magnitude layout between the STFT kernel and its consumers inside the step: 'nfk' bin-fastest (psnd_stft_mag_nfk), 'nkf' the reference's")
    ap.add_argument('--torch-adam', action='store_true', help="torch.optim.Adam(fused=True) instead of pytorch_sound_amd.optim.Adam")
    ap.add_argument('--leg', choices=('config3', 'config4', 'dropin'), help='one bounded single-GPU leg alone, its JSON on stdout (the main run starts each leg this way, in a child process)')
    ap.add_argument('--config', type=int, choices=(2, 3, 4, 5), default=2,
                    help='which BASELINE configuration the contract line runs (1-based as in BASELINE.json configs: 2 = the headline, 3 = conv vocoder DDP, '
                         '4 = transformer block DDP, 5 = 4096-point STFT of 30-s clips); 3 / 4 / 5 take --gpus N under torch.distributed.run like the headline')
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    # RCCL (this torch build's) writes a five-line version banner to STDOUT when the process exits - behind the JSON line - unless its log level is
    # set: rank 0's line must be the last thing on stdout (a caller that wants RCCL's messages sets NCCL_DEBUG itself)
    os.environ.setdefault('NCCL_DEBUG', 'NONE')
    if args.leg:
        if not torch.cuda.is_available():
            raise SystemExit('bench.py needs an MI355X: no GPU visible')
        torch.cuda.set_device(0)
        print(json.dumps({'config3': _config3_leg, 'config4': _config4_leg, 'dropin': _dropin_leg}[args.leg](torch.device('cuda', 0))), flush=True)
        return
    if os.environ.get('PSND_BENCH_WATCHDOG'):      # debugging aid: dump every thread's stack and exit if the run is still alive after S seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ['PSND_BENCH_WATCHDOG']), exit=True)
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X: no GPU visible (there is no CPU fallback for the product path)')
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves (one process per GPU over RCCL, rendezvous on 127.0.0.1) with the
        # same arguments; rank 0 of the children prints the one JSON line, which passes through on our stdout
        import socket
        import subprocess
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
               '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.call(cmd))
    if args.config != 2:
        _emit_line(config_bench(args))
        return
    out, device = gpu_bench(args)
    if out is not None:
        if args.full and args.gpus == 1 and args.cpu_seconds > 0:
            out['cpu_baseline'] = cpu_baseline(args.cpu_seconds * 0.6, 'port')
            out['cpu_baseline_torch_stft'] = cpu_baseline(args.cpu_seconds * 0.4, 'torch_stft')
    _emit_line(out)


if __name__ == '__main__':
    main()
