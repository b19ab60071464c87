"""Times separator -> waveform -> waveform-domain loss at the config-2 geometry (32 clips x 44100 samples, STFT 1024 / 256,
conv_separator_voicebank under bf16 autocast), forward + backward of multi_stft_loss(estimate, clean), on a HIP device:

    separate   ConvSeparator.separate: one STFT launch (|X|, Re X, Im X), mask logits, kernels.istft_reim (sigmoid and product in the
               kernel; backward psnd_istft_reim_bwd: three launches)
    composed   the reference's way: STFT.transform -> model.forward (mask * |X|) -> STFT.inverse (kernels.IStft, whose backward is
               written in ATen ops)

    python tools/time_separate.py [--steps 20] [--rounds 5] [--warmup 10]

Both paths share one model and one input in the same process; both are warmed, then timed in alternation: `rounds` blocks of `steps`
forward + backward passes each, host wall time around a block that ends in a device synchronise.  Prints the mean ms per pass and the
per-block range of both paths, then one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_sound_amd.models import build_model                                      # noqa: E402
from pytorch_sound_amd.models import separator  # noqa: E402,F401
from pytorch_sound_amd.models.sound import multi_stft_loss                            # noqa: E402
from pytorch_sound_amd.models.transforms import STFT                                  # noqa: E402

N, T, N_FFT, HOP = 32, 44100, 1024, 256
LOSS_PARAMS = [(1024, 1024, 256), (2048, 2048, 512), (512, 512, 128)]                 # (n_fft, window, hop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20, help='forward + backward passes per timed block')
    ap.add_argument('--rounds', type=int, default=5, help='timed blocks per path, alternating')
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('no HIP device: nothing is timed on the CPU')
    dev = torch.device('cuda', 0)
    torch.manual_seed(1234)
    model = build_model('conv_separator_voicebank').to(dev).train()
    stft = STFT(N_FFT, HOP).to(dev)
    g = torch.Generator().manual_seed(1)
    noisy = (torch.randn(N, T, generator=g) * 0.1).to(dev)
    L = (T // HOP) * HOP
    clean = (torch.randn(N, T, generator=g) * 0.1).to(dev)[:, :L].contiguous()

    def separate():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            return model.separate(noisy, stft)

    def composed():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            mag, phase = stft.transform(noisy)
            est = model(mag)
        return stft.inverse(est.float(), phase)

    paths = {'separate': separate, 'composed': composed}

    def run(fn, n):
        for _ in range(n):
            model.zero_grad(set_to_none=True)
            multi_stft_loss(fn(), clean, LOSS_PARAMS)[0].backward()

    with torch.no_grad():
        diff = float((separate() - composed()).abs().max())
    for fn in paths.values():
        run(fn, a.warmup)
    torch.cuda.synchronize()
    blocks = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(fn, a.steps)
            torch.cuda.synchronize()
            blocks[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    rows = {}
    for k, b in blocks.items():
        rows[k] = {'ms_per_pass': sum(b) / len(b), 'block_min_ms': min(b), 'block_max_ms': max(b), 'blocks': b}
        print('%-10s %8.3f ms/pass   blocks %.3f .. %.3f' % (k, rows[k]['ms_per_pass'], min(b), max(b)))
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'N': N, 'T': T, 'n_fft': N_FFT, 'hop': HOP, 'steps_per_block': a.steps,
                      'rounds': a.rounds, 'warmup': a.warmup, 'max_abs_difference_of_the_two_waveforms': diff, 'rows': rows}))


if __name__ == '__main__':
    main()
