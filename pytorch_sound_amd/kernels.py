"""Thin torch-tensor front end of the C ABI (include/psnd.h).

PyTorch is plumbing here: it owns device memory and streams; every number is produced
by libpsnd_hip.so.  No function in this module has a CPU or eager fallback - a CPU tensor
or a missing library raises.  (`lfilter`, `resample_poly`, `silence_ranges`, `yin_f0`, `phase_vocoder`, the `griffinlim*` functions, `mel_inverse`, `loudness`, `level`, `apply_gain`, `sep_metric` and `mix_at_snr` alone also take CPU tensors: there the
scipy call or the numpy restatement IS the implementation or the definition; a HIP tensor never reaches it.)
"""
import ctypes
import math
import os
from pytorch_sound_amd import _switches as _sw
import numpy as np
import torch

from . import _lib
from ._lib import PsndError  # noqa: F401
from ._lib import lib, check, ptr, stream_ptr, on, FRAMING_CENTER, FRAMING_HIFIGAN, FRAMING_NONE, LOG_NONE, LOG_E, LOG_10  # noqa: F401

_INF = float('inf')

# bench.py sets this to a list to collect (start, end) HIP event pairs recorded on the launch stream directly
# around every psnd_stft_fwd call (magnitude-only launches), i.e. without the Python work around it.
STFT_FWD_EVENTS = None
STFT_NFK_EVENTS = None          # the same for psnd_stft_mag_nfk


def _need_cuda(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.PsndError('%s must be a CUDA(HIP) tensor: the MI355X path has no CPU fallback' % name)
    if t.dtype != torch.float32:
        raise _lib.PsndError('%s must be float32, got %s' % (name, t.dtype))


def plan_tensor(plan_np):
    """host plan (numpy uint8) -> torch uint8 tensor (CPU); callers register it as a buffer so
    Module.to(device) carries it to the GPU."""
    return torch.from_numpy(np.ascontiguousarray(plan_np))


PLAN_POW2, PLAN_MR = 'pow2', 'mixed-radix'
_MR_BYTES = {}


def _mr_plan_bytes(n_fft):
    nb = _MR_BYTES.get(n_fft)
    if nb is None:
        nb = _MR_BYTES[n_fft] = int(lib().psnd_stft_mr_plan_bytes(int(n_fft)))
    return nb


def stft_plan(n_fft, window):
    """plan of the STFT kernels for this n_fft: a power of two gets the plan of psnd_stft_* as ever, an even 2^a 3^b 5^c up to 4096 the
    plan of the mixed-radix kernels (psnd_stft_mr_*).  The tensor carries `psnd_plan_kind`; that attribute does not survive `.to(device)`,
    so the launchers tell the kinds apart by stft_plan_kind: the two plans of one n_fft never coexist and their sizes are fixed by n_fft."""
    n_fft = int(n_fft)
    if _mr_plan_bytes(n_fft) > 0:
        plan = plan_tensor(_lib.build_stft_mr_plan(n_fft, window))
        plan.psnd_plan_kind = PLAN_MR
        return plan
    if int(lib().psnd_stft_plan_bytes(n_fft)) == 0:
        raise _lib.PsndError('stft plan: n_fft=%d unsupported: the STFT kernels cover powers of two in [16, 8192] and %s'
                             % (n_fft, _lib.STFT_MR_SIZES))
    plan = plan_tensor(_lib.build_stft_plan(n_fft, window))
    plan.psnd_plan_kind = PLAN_POW2
    return plan


def stft_plan_kind(plan, n_fft):
    """PLAN_MR / PLAN_POW2 of a plan built by stft_plan(n_fft, ...), on any device"""
    nb = _mr_plan_bytes(int(n_fft))
    return PLAN_MR if nb > 0 and plan.numel() * plan.element_size() == nb else PLAN_POW2


def _plan_bytes(plan):
    return int(plan.numel() * plan.element_size())


def mel_plan(mel_filter):
    return plan_tensor(_lib.build_mel_plan(mel_filter))


def frame_count(T, n_fft, hop, framing=FRAMING_CENTER):
    return _lib.frame_count(T, n_fft, hop, framing)


def _out_tensor(out, shape, device, what, ok=True):
    """the output tensor of a launch: a new one, or the caller's `out` (a persistent buffer) once it is seen to be what the kernel writes"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if not ok or tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != device or not out.is_contiguous():
        raise _lib.PsndError('%s must be a contiguous fp32 (%d, %d, %d) tensor on %s' % ((what,) + shape + (device,)))
    return out


def _timed(events, N, launch, *args):
    """launch(*args); with `events` a list (STFT_FWD_EVENTS / STFT_NFK_EVENTS) between a pair of timing events recorded on the launch
    stream directly around it - not inside a hipGraph capture"""
    if events is None or torch.cuda.is_current_stream_capturing():
        return launch(*args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch(*args)
    e1.record()
    events.append((e0, e1, N))


def _scratch(nbytes, device):
    """(scratch tensor, its size in bytes) as the entry points with a scratch take them"""
    scratch = torch.empty(max(int(nbytes) // 4, 1), dtype=torch.float32, device=device)
    return scratch, scratch.numel() * 4


_MR_ENTRY = {'psnd_stft_fwd': 'psnd_stft_mr_fwd', 'psnd_stft_bwd': 'psnd_stft_mr_bwd', 'psnd_istft': 'psnd_istft_mr',
             'psnd_istft_reim': 'psnd_istft_reim_mr'}


def _plan_launch(hip, name, plan, n_fft, mr_scratch=None):
    """the two plan kinds behind one name: (launch, plan arguments, scratch arguments) of entry point `name` for this plan.  A power-of-two
    plan is passed alone and needs no scratch; the mixed-radix twin takes the plan with its size and, where it works through a scratch,
    the `_scratch` that `mr_scratch()` allocates."""
    if stft_plan_kind(plan, n_fft) != PLAN_MR:
        return getattr(hip, name), (plan,), ()
    return getattr(hip, _MR_ENTRY[name]), (plan, _plan_bytes(plan)), mr_scratch() if mr_scratch else ()


def stft_forward(wav, n_fft, hop, plan, framing=FRAMING_CENTER, mag_eps=0.0,
                 want_mag=True, want_phase=False, want_reim=False, out_mag=None):
    """wav (N,T) fp32 cuda -> dict of requested (N,K,F) tensors.  out_mag: a caller-owned (N,K,F) fp32 tensor the magnitude is written
    into (feature extraction into persistent buffers, Trainer.static_prepare)."""
    _need_cuda(wav, 'wav')
    if wav.dim() != 2:
        raise _lib.PsndError('wav must be (N, T), got %s' % (tuple(wav.shape),))
    if plan.device != wav.device:
        raise _lib.PsndError('stft plan lives on %s but wav on %s (move the module with .to())' % (plan.device, wav.device))
    wav = wav.contiguous()
    N, T = wav.shape
    F = frame_count(T, n_fft, hop, framing)
    K = n_fft // 2 + 1
    mk = lambda: torch.empty((N, K, F), dtype=torch.float32, device=wav.device)  # noqa: E731
    if want_mag or out_mag is not None:
        mag = _out_tensor(out_mag, (N, K, F), wav.device, 'stft_forward: out_mag', ok=want_mag)
    else:
        mag = None
    phase = mk() if want_phase else None
    re = mk() if want_reim else None
    im = mk() if want_reim else None
    with on(wav.device) as hip:
        launch, plan_args, _ = _plan_launch(hip, 'psnd_stft_fwd', plan, n_fft)
        _timed(STFT_FWD_EVENTS, N, launch, wav, N, T, n_fft, hop, framing, *plan_args, float(mag_eps), mag, phase, re, im)
    return {'mag': mag, 'phase': phase, 're': re, 'im': im}


def stft_mag_nfk(wav, n_fft, hop, plan, framing=FRAMING_CENTER, mag_eps=0.0, out=None):
    """psnd_stft_mag_nfk: wav (N,T) fp32 -> magnitude (N, F, K), bin axis fastest (`.transpose(1, 2)` is the reference's (N, K, F)
    as a view).  For consumers inside this library that take the layout (mel kernel, channels-last conv stack); no autograd."""
    _need_cuda(wav, 'wav')
    if wav.dim() != 2:
        raise _lib.PsndError('wav must be (N, T), got %s' % (tuple(wav.shape),))
    if plan.device != wav.device:
        raise _lib.PsndError('stft plan lives on %s but wav on %s (move the module with .to())' % (plan.device, wav.device))
    wav = wav.detach().contiguous()
    N, T = wav.shape
    F = frame_count(T, n_fft, hop, framing)
    K = n_fft // 2 + 1
    out = _out_tensor(out, (N, F, K), wav.device, 'stft_mag_nfk: out')
    with on(wav.device) as hip:
        _timed(STFT_NFK_EVENTS, N, hip.psnd_stft_mag_nfk, wav, N, T, n_fft, hop, framing, plan, float(mag_eps), out)
    return out


def stft_backward(wav, n_fft, hop, plan, framing=FRAMING_CENTER, mag_eps=0.0, gmag=None, gre=None, gim=None):
    _need_cuda(wav, 'wav')
    wav = wav.contiguous()
    N, T = wav.shape
    gs = [None if g is None else g.contiguous() for g in (gmag, gre, gim)]
    for g in gs:
        if g is not None:
            _need_cuda(g, 'grad')
    gwav = torch.empty_like(wav)
    with on(wav.device) as hip:
        # mixed radix: two launches, the windowed frame gradients go through a scratch, every sample gathers its frames in a fixed order
        launch, plan_args, scratch = _plan_launch(hip, 'psnd_stft_bwd', plan, n_fft, lambda: _scratch(
            lib().psnd_stft_mr_bwd_scratch_bytes(N, T, n_fft, hop, framing), wav.device))
        launch(wav, N, T, n_fft, hop, framing, *plan_args, float(mag_eps), *gs, *scratch, gwav)
    return gwav


def _clamp_args(clamp_lo, clamp_hi, pre_clamp_min):
    lo = -_INF if clamp_lo is None else float(clamp_lo)
    hi = _INF if clamp_hi is None else float(clamp_hi)
    pre = -1.0 if pre_clamp_min is None else float(pre_clamp_min)
    return lo, hi, pre


def mel_forward(mag, mel_plan_t, M, log_kind=LOG_E, log_offset=0.0, pre_clamp_min=None,
                clamp_lo=None, clamp_hi=None, want_lin=False, out=None):
    _need_cuda(mag, 'mag')
    mag = mag.contiguous()
    N, K, F = mag.shape
    lo, hi, pre = _clamp_args(clamp_lo, clamp_hi, pre_clamp_min)
    out = _out_tensor(out, (N, M, F), mag.device, 'mel_forward: out')
    lin = torch.empty_like(out) if want_lin else None
    with on(mag.device) as hip:
        hip.psnd_mel_fwd(mag, N, F, M, K, mel_plan_t, log_kind, float(log_offset), pre, lo, hi, out, lin)
    return out, lin


def mel_forward_nfk(mag_nfk, mel_plan_t, M, log_kind=LOG_E, log_offset=0.0, pre_clamp_min=None, clamp_lo=None, clamp_hi=None,
                    want_lin=False, out=None):
    """psnd_mel_fwd_nfk: the mel projection of a BIN-FASTEST magnitude (N, F, K) (stft_mag_nfk); the result is (N, M, F) as mel_forward's"""
    _need_cuda(mag_nfk, 'mag_nfk')
    mag_nfk = mag_nfk.contiguous()
    N, F, K = mag_nfk.shape
    lo, hi, pre = _clamp_args(clamp_lo, clamp_hi, pre_clamp_min)
    out = _out_tensor(out, (N, M, F), mag_nfk.device, 'mel_forward_nfk: out')
    lin = torch.empty_like(out) if want_lin else None
    with on(mag_nfk.device) as hip:
        hip.psnd_mel_fwd_nfk(mag_nfk, N, F, M, K, mel_plan_t, log_kind, float(log_offset), pre, lo, hi, out, lin)
    return out, lin


def mel_backward_nfk(gout, mel_lin, mel_plan_t, K, log_kind=LOG_E, log_offset=0.0, pre_clamp_min=None, clamp_lo=None, clamp_hi=None):
    """psnd_mel_bwd_nfk: gradient of mel_forward_nfk w.r.t. the magnitude, (N, F, K)"""
    _need_cuda(gout, 'gout')
    gout = gout.contiguous()
    N, M, F = gout.shape
    lo, hi, pre = _clamp_args(clamp_lo, clamp_hi, pre_clamp_min)
    gmag = torch.empty((N, F, K), dtype=torch.float32, device=gout.device)
    with on(gout.device) as hip:
        hip.psnd_mel_bwd_nfk(gout, mel_lin, N, F, M, K, mel_plan_t, log_kind, float(log_offset), pre, lo, hi, gmag)
    return gmag


class MelLogNfk(torch.autograd.Function):
    """MelLog for a bin-fastest magnitude: (N, F, K) -> (N, M, F)"""

    @staticmethod
    def forward(ctx, mag_nfk, plan, M, log_kind, log_offset, pre_clamp_min, clamp_lo, clamp_hi):
        need_grad = ctx.needs_input_grad[0]
        out, lin = mel_forward_nfk(mag_nfk, plan, M, log_kind, log_offset, pre_clamp_min, clamp_lo, clamp_hi, want_lin=need_grad)
        if need_grad:
            ctx.save_for_backward(lin, plan)
        ctx.cfg = (mag_nfk.shape[2], log_kind, log_offset, pre_clamp_min, clamp_lo, clamp_hi)
        return out

    @staticmethod
    def backward(ctx, gout):
        lin, plan = ctx.saved_tensors
        K, log_kind, log_offset, pre, lo, hi = ctx.cfg
        return mel_backward_nfk(gout, lin, plan, K, log_kind, log_offset, pre, lo, hi), None, None, None, None, None, None, None


def logmel_fused_ok(wav, n_fft, hop):
    """the fused wav -> log-mel kernel covers the span-staged tile size and needs no gradient (forward only)"""
    return (n_fft == 1024 and 0 < hop <= 256 and hop % 4 == 0 and wav.is_cuda
            and not (torch.is_grad_enabled() and wav.requires_grad))


def logmel_forward(wav, n_fft, hop, stft_plan_t, mel_plan_t, M, framing=FRAMING_CENTER, mag_eps=0.0, log_kind=LOG_E,
                   log_offset=0.0, pre_clamp_min=None, clamp_lo=None, clamp_hi=None):
    """psnd_logmel_fwd: (N,T) waveform -> (N,M,F) log-mel, magnitude kept on chip"""
    _need_cuda(wav, 'wav')
    wav = wav.detach().contiguous()
    N, T = wav.shape
    F = frame_count(T, n_fft, hop, framing)
    lo, hi, pre = _clamp_args(clamp_lo, clamp_hi, pre_clamp_min)
    out = torch.empty((N, M, max(F, 0)), dtype=torch.float32, device=wav.device)
    with on(wav.device) as hip:
        hip.psnd_logmel_fwd(wav, N, T, n_fft, hop, framing, stft_plan_t, float(mag_eps), M, mel_plan_t, log_kind, float(log_offset), pre, lo, hi, out)
    return out


def mel_backward(gout, mel_lin, mel_plan_t, K, log_kind=LOG_E, log_offset=0.0, pre_clamp_min=None,
                 clamp_lo=None, clamp_hi=None):
    _need_cuda(gout, 'gout')
    gout = gout.contiguous()
    N, M, F = gout.shape
    lo, hi, pre = _clamp_args(clamp_lo, clamp_hi, pre_clamp_min)
    gmag = torch.empty((N, K, F), dtype=torch.float32, device=gout.device)
    with on(gout.device) as hip:
        hip.psnd_mel_bwd(gout, mel_lin, N, F, M, K, mel_plan_t, log_kind, float(log_offset), pre, lo, hi, gmag)
    return gmag


# ---------------------------------------------------------------------------------------------
# autograd glue
# ---------------------------------------------------------------------------------------------
class StftMagPhase(torch.autograd.Function):
    """(mag, phase) of STFT.transform (transforms.py:53-69).  phase is detached there
    (atan2 of .data) -> marked non-differentiable here."""

    @staticmethod
    def forward(ctx, wav, plan, n_fft, hop, framing, mag_eps, want_phase):
        o = stft_forward(wav, n_fft, hop, plan, framing, mag_eps, True, want_phase, False)
        ctx.save_for_backward(wav, plan)
        ctx.cfg = (n_fft, hop, framing, mag_eps)
        if want_phase:
            ctx.mark_non_differentiable(o['phase'])
            return o['mag'], o['phase']
        return o['mag'], None

    @staticmethod
    def backward(ctx, gmag, _gphase):
        wav, plan = ctx.saved_tensors
        n_fft, hop, framing, mag_eps = ctx.cfg
        gw = stft_backward(wav, n_fft, hop, plan, framing, mag_eps, gmag=gmag)
        return gw, None, None, None, None, None, None


class StftReIm(torch.autograd.Function):
    """(re, im) of torch.stft as STFTTorchAudio.forward uses it (transforms.py:297-303); both
    outputs are differentiable (transform() there does NOT detach the phase, :311)."""

    @staticmethod
    def forward(ctx, wav, plan, n_fft, hop, framing):
        o = stft_forward(wav, n_fft, hop, plan, framing, 0.0, False, False, True)
        ctx.save_for_backward(wav, plan)
        ctx.cfg = (n_fft, hop, framing)
        return o['re'], o['im']

    @staticmethod
    def backward(ctx, gre, gim):
        wav, plan = ctx.saved_tensors
        n_fft, hop, framing = ctx.cfg
        if gre is None:
            gre = torch.zeros_like(gim)
        if gim is None:
            gim = torch.zeros_like(gre)
        gw = stft_backward(wav, n_fft, hop, plan, framing, 0.0, gre=gre, gim=gim)
        return gw, None, None, None, None


class StftPolar(torch.autograd.Function):
    """(magnitude, phase) of STFTTorchAudio.transform (transforms.py:305-311): both outputs come out of ONE psnd_stft_fwd launch and
    both are differentiable (the reference takes atan2 of the live tensors there).  Backward: a magnitude-only gradient takes the
    tuned magnitude adjoint; with a phase gradient, psnd_polar_bwd turns (g_mag, g_phase) into (g_re, g_im) in one pass and the
    (re, im) adjoint carries on."""

    @staticmethod
    def forward(ctx, wav, plan, n_fft, hop, framing):
        o = stft_forward(wav, n_fft, hop, plan, framing, 0.0, True, True, False)
        ctx.save_for_backward(wav, plan, o['mag'], o['phase'])
        ctx.cfg = (n_fft, hop, framing)
        return o['mag'], o['phase']

    @staticmethod
    def backward(ctx, gmag, gphase):
        wav, plan, mag, phase = ctx.saved_tensors
        n_fft, hop, framing = ctx.cfg
        if gphase is None:
            return stft_backward(wav, n_fft, hop, plan, framing, 0.0, gmag=gmag), None, None, None, None
        gphase = gphase.contiguous()
        gmag = None if gmag is None else gmag.contiguous()
        gre, gim = torch.empty_like(mag), torch.empty_like(mag)
        with on(mag.device) as hip:
            hip.psnd_polar_bwd(gmag, gphase, mag, phase, mag.numel(), gre, gim)
        return stft_backward(wav, n_fft, hop, plan, framing, 0.0, gre=gre, gim=gim), None, None, None, None


class MelLog(torch.autograd.Function):
    """clamp(log(max(W @ mag, pre) + off), lo, hi) - transforms.py:235-243 / :364-365 /
    interface/hifi_gan.py:58-61."""

    @staticmethod
    def forward(ctx, mag, plan, M, log_kind, log_offset, pre_clamp_min, clamp_lo, clamp_hi):
        need_grad = ctx.needs_input_grad[0]
        out, lin = mel_forward(mag, plan, M, log_kind, log_offset, pre_clamp_min, clamp_lo, clamp_hi, want_lin=need_grad)
        if need_grad:
            ctx.save_for_backward(lin, plan)
        ctx.cfg = (mag.shape[1], log_kind, log_offset, pre_clamp_min, clamp_lo, clamp_hi)
        return out

    @staticmethod
    def backward(ctx, gout):
        lin, plan = ctx.saved_tensors
        K, log_kind, log_offset, pre, lo, hi = ctx.cfg
        gmag = mel_backward(gout, lin, plan, K, log_kind, log_offset, pre, lo, hi)
        return gmag, None, None, None, None, None, None, None


def db_to_ln(db):
    """np.log(np.power(10, db / 10)) of transforms.py:223,227"""
    return math.log(math.pow(10.0, db / 10.0))


def istft_forward(magnitude, phase, n_fft, hop, plan, eps=1e-9):
    _need_cuda(magnitude, 'magnitude')
    _need_cuda(phase, 'phase')
    magnitude, phase = magnitude.contiguous(), phase.contiguous()
    N, Kb, F = magnitude.shape
    if Kb != n_fft // 2 + 1 or phase.shape != magnitude.shape:
        raise _lib.PsndError('istft: expected (N, %d, F) magnitude and phase, got %s / %s'
                             % (n_fft // 2 + 1, tuple(magnitude.shape), tuple(phase.shape)))
    out = torch.empty((N, max((F - 1) * hop, 0)), dtype=torch.float32, device=magnitude.device)
    with on(magnitude.device) as hip:
        launch, plan_args, scratch = _plan_launch(hip, 'psnd_istft', plan, n_fft, lambda: _scratch(
            lib().psnd_istft_mr_scratch_bytes(N, F, n_fft), magnitude.device))
        launch(magnitude, phase, N, F, n_fft, hop, *plan_args, float(eps), *scratch, out)
    return out


_OLA_ENV = {}


def _ola_envelope(window, n_fft, hop, F):
    """sum_f window^2[t - f hop] over F frames, length (F - 1) hop + n_fft - the overlap-add envelope STFT.inverse divides by
    (transforms.py:90-99 builds it with a conv_transpose1d of ones; here ceil(n_fft / hop) shifted block adds, cached per window / geometry:
    no library convolution for a HIP tensor)."""
    import weakref
    key = (id(window), window._version, n_fft, hop, F)
    hit = _OLA_ENV.get(key)
    env = hit[1] if hit is not None and hit[0]() is window else None      # the id of a freed tensor may be reused: the weak reference tells
    if env is None:
        if len(_OLA_ENV) > 32:
            _OLA_ENV.clear()
        # deterministic: the window squared cut into R = ceil(n_fft / hop) pieces of `hop` samples; piece r of every frame lands on the hop
        # blocks r .. r + F - 1, added piece by piece in a fixed order (an index_add_ of F shifted copies adds with float atomics)
        w2 = (window.detach().float() * window.detach().float()).reshape(-1)
        R = (n_fft + hop - 1) // hop
        w2 = torch.nn.functional.pad(w2, (0, R * hop - n_fft)).view(R, hop)
        blocks = torch.zeros((F - 1 + R, hop), dtype=torch.float32, device=window.device)
        for r in range(R):
            blocks[r:r + F] += w2[r]
        env = blocks.reshape(-1)[:(F - 1) * hop + n_fft].contiguous()
        _OLA_ENV[key] = (weakref.ref(window), env)
    return env


class IStft(torch.autograd.Function):
    """STFT.inverse (transforms.py:71-101).  Backward: the map is linear in G = s_k * mag * e^{i phase}
    (s = 1/n for DC/Nyquist, 2/n otherwise; their imaginary parts do not reach the signal), and its adjoint is a
    plain windowed forward DFT (no padding) of the envelope-scaled output gradient - psnd_stft_fwd again."""

    @staticmethod
    def forward(ctx, magnitude, phase, window, plan, n_fft, hop, eps):
        out = istft_forward(magnitude, phase, n_fft, hop, plan, eps)
        ctx.save_for_backward(magnitude, phase, window, plan)
        ctx.cfg = (n_fft, hop, eps)
        return out

    @staticmethod
    def backward(ctx, g):
        magnitude, phase, window, plan = ctx.saved_tensors
        n_fft, hop, eps = ctx.cfg
        N, Kb, F = magnitude.shape
        env = _ola_envelope(window, n_fft, hop, F)
        p = n_fft // 2
        gp = torch.nn.functional.pad(g.contiguous(), (p, p))
        den = env + eps
        # eps = 0 (torch.istft's convention): the envelope vanishes only inside the trimmed n/2 edges, where the gradient is zero too
        gp = torch.where(den > 0, gp / den, torch.zeros_like(gp))
        o = stft_forward(gp, n_fft, hop, plan, FRAMING_NONE, 0.0, False, False, True)
        s = torch.full((Kb,), 2.0 / n_fft, device=g.device)
        s[0] = s[-1] = 1.0 / n_fft
        are, aim = o['re'] * s.view(1, -1, 1), o['im'] * s.view(1, -1, 1)
        aim[:, 0] = 0
        aim[:, -1] = 0
        cs, sn = torch.cos(phase), torch.sin(phase)
        g_mag = cs * are + sn * aim
        g_phase = magnitude * (cs * aim - sn * are)
        return g_mag, g_phase, None, None, None, None, None


def istft(magnitude, phase, n_fft, hop, plan, eps=1e-9, window=None):
    """STFT.inverse - differentiable when `window` (n_fft taps, on the device) is given."""
    if window is not None and (magnitude.requires_grad or phase.requires_grad):
        return IStft.apply(magnitude, phase, window, plan, n_fft, hop, eps)
    return istft_forward(magnitude, phase, n_fft, hop, plan, eps)


# ---------------------------------------------------------------------------------------------
# masked inverse STFT on (re, im): psnd_istft_reim / _reim_mr / _reim_bwd
# ---------------------------------------------------------------------------------------------
MASK_NONE, MASK_LINEAR, MASK_SIGMOID = _lib.MASK_NONE, _lib.MASK_LINEAR, _lib.MASK_SIGMOID


def _reim_args(re, im, mask, mask_kind, n_fft):
    _need_cuda(re, 're')
    _need_cuda(im, 'im')
    if re.dim() != 3 or re.shape[1] != n_fft // 2 + 1 or im.shape != re.shape:
        raise _lib.PsndError('istft_reim: expected (N, %d, F) re and im, got %s / %s' % (n_fft // 2 + 1, tuple(re.shape), tuple(im.shape)))
    if mask_kind not in (MASK_NONE, MASK_LINEAR, MASK_SIGMOID) or (mask is None) != (mask_kind == MASK_NONE):
        raise _lib.PsndError('istft_reim: mask_kind=%r %s a mask' % (mask_kind, 'without' if mask is None else 'with'))
    if mask is not None:
        _need_cuda(mask, 'mask')
        if mask.shape != re.shape:
            raise _lib.PsndError('istft_reim: mask %s does not match the spectrum %s' % (tuple(mask.shape), tuple(re.shape)))
        mask = mask.contiguous()
    return re.contiguous(), im.contiguous(), mask


def istft_reim_forward(re, im, mask, mask_kind, n_fft, hop, plan, eps=1e-9):
    """the waveform of the spectrum m (re + i im), (N, (F - 1) hop): psnd_istft's definition without the polar round trip"""
    re, im, mask = _reim_args(re, im, mask, mask_kind, n_fft)
    N, _, F = re.shape
    out = torch.empty((N, max((F - 1) * hop, 0)), dtype=torch.float32, device=re.device)
    with on(re.device) as hip:
        launch, plan_args, scratch = _plan_launch(hip, 'psnd_istft_reim', plan, n_fft, lambda: _scratch(
            lib().psnd_istft_mr_scratch_bytes(N, F, n_fft), re.device))
        launch(re, im, mask, mask_kind, N, F, n_fft, hop, *plan_args, float(eps), *scratch, out)
    return out


def istft_reim_backward(g, re, im, mask, mask_kind, n_fft, hop, plan, eps=1e-9, want_reim=True, want_mask=True):
    """(g_re, g_im, g_mask) of istft_reim_forward for the output gradient g, each (N, K, F) or None: three launches (psnd_istft_reim_bwd)"""
    re, im, mask = _reim_args(re, im, mask, mask_kind, n_fft)
    _need_cuda(g, 'g')
    g = g.contiguous()
    N, _, F = re.shape
    if tuple(g.shape) != (N, max((F - 1) * hop, 0)):
        raise _lib.PsndError('istft_reim_backward: g %s is not the (N, (F - 1) hop) = (%d, %d) output gradient' % (tuple(g.shape), N, (F - 1) * hop))
    want_mask = want_mask and mask is not None
    # F <= 1: the output is empty and the entry point launches nothing, so the gradients are allocated as zeros
    mk = torch.zeros_like if F <= 1 or N == 0 else torch.empty_like
    g_re = mk(re) if want_reim else None
    g_im = mk(re) if want_reim else None
    g_mask = mk(re) if want_mask else None
    if not want_reim and not want_mask:
        return None, None, None
    scratch = _scratch(lib().psnd_istft_reim_bwd_scratch_bytes(N, F, n_fft), re.device)
    with on(re.device) as hip:      # one entry point for both plan kinds
        hip.psnd_istft_reim_bwd(g, re, im, mask, mask_kind, N, F, n_fft, hop, plan, _plan_bytes(plan), float(eps), *scratch, g_re, g_im, g_mask)
    return g_re, g_im, g_mask


class IStftReIm(torch.autograd.Function):
    """istft_reim: the inverse STFT of m (re + i im).  Both directions are kernels of the library - inside this node no ATen compute op
    touches a HIP tensor, only allocations."""

    @staticmethod
    def forward(ctx, re, im, mask, plan, mask_kind, n_fft, hop, eps):
        out = istft_reim_forward(re, im, mask, mask_kind, n_fft, hop, plan, eps)
        ctx.save_for_backward(re, im, mask, plan)
        ctx.cfg = (mask_kind, n_fft, hop, eps)
        return out

    @staticmethod
    def backward(ctx, g):
        re, im, mask, plan = ctx.saved_tensors
        mask_kind, n_fft, hop, eps = ctx.cfg
        need = ctx.needs_input_grad
        g_re, g_im, g_mask = istft_reim_backward(g, re, im, mask, mask_kind, n_fft, hop, plan, eps, need[0] or need[1], need[2])
        return (g_re if need[0] else None), (g_im if need[1] else None), g_mask, None, None, None, None, None


def istft_reim(re, im, mask, mask_kind, n_fft, hop, plan, eps=1e-9):
    """waveform (N, (F - 1) hop) of the spectrum m (re + i im); m = 1 (MASK_NONE, mask None), the mask (MASK_LINEAR) or sigmoid(mask)
    (MASK_SIGMOID, evaluated in the kernel).  Differentiable in re, im and mask; the plan kind is told by stft_plan_kind."""
    if mask_kind is None:
        mask_kind = MASK_NONE if mask is None else MASK_LINEAR
    if torch.is_grad_enabled() and (re.requires_grad or im.requires_grad or (mask is not None and mask.requires_grad)):
        return IStftReIm.apply(re, im, mask, plan, mask_kind, n_fft, hop, eps)
    return istft_reim_forward(re, im, mask, mask_kind, n_fft, hop, plan, eps)


# ---------------------------------------------------------------------------------------------
# transformer blocks (models/modules.py): GroupNorm(1, C)(x + res) and the masked softmax over keys
# ---------------------------------------------------------------------------------------------
RESIDUAL_LINKS = _sw.lab('PSND_RESIDUAL_LINKS', '1') == '1'      # 0: autograd accumulates the two gradients of a block's input (A/B)


class ResidualLink:
    """One residual connection y = norm(f(x) + x) whose branch f starts with a Linear1x1 on the same x (MultiHeadAttention,
    PointwiseFeedForward): autograd would add the two gradients of x in a pass of its own (three tensor sweeps); instead the norm's
    backward hands its gradient for x to the link and returns none, and the Linear1x1's backward - which runs later in the same pass and
    consumes it - writes W^T gy + that gradient (psnd_linear1x1_bwd_acc).  The projection registers itself when its forward was recorded
    with x requiring a gradient; without a registered consumer the norm returns its gradient as usual."""

    def __init__(self):
        self.consumer = False      # a Linear1x1 node that will produce a gradient for x holds this link
        self.g = None

    def offer(self, g) -> bool:
        if not self.consumer or not RESIDUAL_LINKS:
            return False
        self.g = g
        return True

    def take(self):
        g, self.g = self.g, None
        return g


RELU_LINKS = _sw.lab('PSND_RELU_LINKS', '1') == '1'              # 0: each GEMM behind the ReLU masks its operand itself (A/B)


PAD_HIDDEN_ROWS = _sw.lab('PSND_FFN_PAD_ROWS', '1') == '1'       # 0: the bf16 hidden tensor's rows are T frames long (A/B)
HIDDEN_BF16 = _sw.lab('PSND_FFN_HIDDEN_BF16', '1') == '1'      # 0: the feed-forward pair's hidden tensor stays fp32 under autocast (A/B)


class ReluLink:
    """Conv1d -> ReLU -> Conv1d (PointwiseFeedForward, modules.py:93-95) as two Linear1x1 nodes: the first one's backward would read
    its incoming gradient together with the ReLU's output as a mask in both of its GEMMs and its bias sum (two 169 MB tensors each at 32
    clips x 1292 frames x 1024 channels).  With a link the SECOND node, which produces that gradient and holds the ReLU's output as its
    input, zeroes it where the ReLU was off in its GEMM's epilogue (psnd_linear1x1_bwd_ex, gx_mask), says so here, and the first node
    reads the gradient alone.  The values are the same either way (a masked element is an exact zero in both)."""

    def __init__(self):
        self.consumer = False      # the second node was recorded on the first one's output and will produce a gradient for it
        self.y = None              # (address, shape) of the ReLU's output as the first node returned it: the second node checks that ITS
                                   # input is that tensor (no reference: the output's grad_fn holds the link)
        self.masked = False        # set by the second node's backward: the gradient arrives masked

    def take(self) -> bool:
        m, self.masked = self.masked, False
        return m


# dropout in front of the norm (modules.py:54-56, :112-114), formed inside the GroupNorm kernels: the mask is a pure function of the element's
# index and of a {seed, call} pair (Philox4x32-10, include/psnd.h), the pair lives in DEVICE memory and every application takes it through
# psnd_rng_next, which counts the call - stream ordered and capturable, so each replay of a step graph draws fresh masks.
_DROPOUT_STATE = {}            # device index -> int64[2] device tensor holding the two uint64 {seed, call}
_U64 = (1 << 64) - 1


def _dropout_device(device):
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != 'cuda':
        raise PsndError('the dropout state lives on a HIP device, got %s' % device)
    return device if device.index is not None else torch.device('cuda', torch.cuda.current_device())


def dropout_seed(seed, call=0, device=None):
    """(re)start the dropout stream of `device` at {seed, call}: a one-thread kernel on the current stream, no synchronisation"""
    device = _dropout_device(device)
    with on(device) as hip:
        st = _DROPOUT_STATE.get(device.index)
        if st is None:
            if torch.cuda.is_current_stream_capturing():
                raise PsndError('dropout on %s: no dropout state yet and a stream capture is under way (the state would live in the graph\'s '
                                'memory) - call pytorch_sound_amd.kernels.dropout_seed(seed) before the capture' % device)
            st = _DROPOUT_STATE[device.index] = torch.empty(2, dtype=torch.int64, device=device)
        hip.psnd_rng_seed(st, int(seed) & _U64, int(call) & _U64)
    return st


def _dropout_state_tensor(device):
    st = _DROPOUT_STATE.get(device.index)
    # first use without seeding: torch.initial_seed() reads the default generator's seed and draws nothing from it
    return st if st is not None else dropout_seed(torch.initial_seed(), 0, device)


def dropout_state(device=None):
    """(seed, call) of the next dropout application on `device` - SYNCHRONISES; for tests and checkpoints"""
    seed, call = _dropout_state_tensor(_dropout_device(device)).cpu().tolist()
    return seed & _U64, call & _U64


def _dropout_reset(device=None):
    """test hook: forget the state of `device`, as in a process that never used dropout"""
    _DROPOUT_STATE.pop(_dropout_device(device).index, None)


def dropout_threshold(p):
    """(thr, scale) of rate p: an element is kept iff its Philox word is >= thr = min(2^32 - 1, floor(p * 2^32)); scale = 1 / (1 - p) in fp32"""
    p = float(p)
    if not 0.0 < p < 1.0 or np.float32(p) >= 1:
        raise PsndError('dropout rate %r: the kernels take 0 < p < 1 (as an fp32 number)' % (p,))
    return min(2 ** 32 - 1, int(math.floor(p * 2.0 ** 32))), float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


class GroupNorm1(torch.autograd.Function):
    """y = GroupNorm(1, C)(x + res) [-> ReLU]: statistics over (C x T) per sample (modules.py:58, :114-116).
    drop = p: y = GroupNorm(1, C)(dropout_p(x) + res) [-> ReLU] in the same two launches (psnd_groupnorm1_drop_*), the mask recomputed
    from the application's {seed, call} pair in every pass."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, relu, link=None, drop=None):
        _need_cuda(x, 'x')
        x = x.contiguous()
        res = None if res is None else res.contiguous()
        ctx.link = link if (link is not None and res is not None) else None
        N, C, T = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((N, 2), dtype=torch.float32, device=x.device)
        ws = torch.empty((N, 2 * C), dtype=torch.float64, device=x.device)         # PSND_GN_WS_DOUBLES(C) per sample: a pair of sums per row
        g32, b32 = gamma.detach().contiguous(), beta.detach().contiguous()
        key = None
        ctx.drop = None if drop is None else dropout_threshold(drop)
        with on(x.device) as hip:
            if ctx.drop is None:
                hip.psnd_groupnorm1_fwd(x, res, g32, b32, N, C, T, float(eps), int(relu), y, stats, ws)
            else:
                state = _dropout_state_tensor(x.device)
                key = torch.empty(2, dtype=torch.int64, device=x.device)           # this application's {seed, call}: backward reads it again
                hip.psnd_rng_next(state, key)
                hip.psnd_groupnorm1_drop_fwd(x, res, g32, b32, N, C, T, float(eps), int(relu), y, stats, ws, key, ctx.drop[0], ctx.drop[1])
        ctx.relu, ctx.has_res = bool(relu), res is not None
        ctx.save_for_backward(x, res, g32, y if relu else None, stats, key)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, res, g32, y, stats, key = ctx.saved_tensors
        gy = gy.contiguous()
        N, C, T = x.shape
        gx = torch.empty_like(x)
        gg = torch.empty(C, dtype=torch.float32, device=x.device)
        gb = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = torch.empty((N, 2 * C), dtype=torch.float64, device=x.device)         # PSND_GN_WS_DOUBLES(C) per sample: a pair of sums per row
        if ctx.drop is not None:
            # two gradients: the sum's (the residual's) and, masked and scaled, x's; the residual's is written only when somebody takes it
            gres = torch.empty_like(x) if (ctx.has_res and ctx.needs_input_grad[1]) else None
            with on(x.device) as hip:
                hip.psnd_groupnorm1_drop_bwd(gy, x, res, g32, y, stats, N, C, T, int(ctx.relu), gx, gres, gg, gb, ws, key, ctx.drop[0], ctx.drop[1])
            if ctx.link is not None and gres is not None and ctx.link.offer(gres):
                return gx, None, gg, gb, None, None, None, None
            return gx, gres, gg, gb, None, None, None, None
        with on(x.device) as hip:
            hip.psnd_groupnorm1_bwd(gy, x, res, g32, y, stats, N, C, T, int(ctx.relu), gx, gg, gb, ws)
        if ctx.link is not None and ctx.needs_input_grad[1] and ctx.link.offer(gx):
            # the residual's gradient travels with the link: the first projection of the branch adds it in its input-gradient GEMM
            return gx, None, gg, gb, None, None, None, None
        return gx, (gx if ctx.has_res else None), gg, gb, None, None, None, None


class SoftmaxKeys(torch.autograd.Function):
    """att = softmax over keys (dim 1) of scale * scores, key-padded rows -> -inf before, query-padded columns -> 0
    after (modules.py:66-76).  In place on `scores` when it is a non-leaf temporary (the bmm output), else on a copy."""

    @staticmethod
    def forward(ctx, scores, mask_u8, scale):
        _need_cuda(scores, 'scores')
        if scores.is_contiguous() and not (scores.is_leaf and scores.requires_grad):
            att = scores                               # the bmm output is a temporary: softmax in place, no extra pass
            ctx.mark_dirty(scores)
        else:
            att = scores.contiguous().clone()
        B, T, _ = att.shape
        with on(att.device) as hip:
            hip.psnd_softmax_keys_fwd(att, mask_u8, B, T, float(scale))
        ctx.scale = float(scale)
        ctx.save_for_backward(att)
        return att

    @staticmethod
    def backward(ctx, gatt):
        (att,) = ctx.saved_tensors
        gatt = gatt.contiguous()
        B, T, _ = att.shape
        gs = torch.empty_like(att)
        with on(att.device) as hip:
            hip.psnd_softmax_keys_bwd(att, gatt, B, T, ctx.scale, gs)
        return gs, None, None


# ---------------------------------------------------------------------------------------------
# models/sound.py: PreEmphasis and multi_stft_loss
# ---------------------------------------------------------------------------------------------
class Linear1x1(torch.autograd.Function):
    """y = W x + b per time step (a 1x1 Conv1d, modules.py:21-22, 93-95) on the matrix-core GEMM (psnd_linear1x1_*): exact fp32
    products, or bf16 operands / fp32 accumulation with `bf16=True`; optionally with the ReLU that follows it fused (its backward
    masks by y > 0).  x: (N, Cin, T), w: (Cout, Cin) or (Cout, Cin, 1); output and gradients fp32."""

    @staticmethod
    def forward(ctx, x, w, bias, relu, bf16=False, link=None, relu_link=None, out_h=False, t_len=None, pad_h=False):
        # t_len: the frames of a row in use when x is a bf16 tensor with padded rows (N, Cin, ld_h >= t_len); pad_h: the bf16 output gets such
        # rows (ld_h = the next multiple of 64 frames: every row starts on a 128-byte line) - a tensor between two nodes of this class only
        # out_h (with bf16 operands): the output is STORED as bf16 - the hidden tensor of Conv1d -> ReLU -> Conv1d under autocast; the node
        # behind it takes it as it is (x.dtype == bfloat16).  The products round their operands to bf16 anyway: same values, half the bytes.
        x_h = x.dtype == torch.bfloat16
        if not (x_h and isinstance(x, torch.Tensor) and x.is_cuda):
            _need_cuda(x, 'input')
        if (x_h or out_h) and not bf16:
            raise PsndError('Linear1x1: bf16 storage comes with bf16 operands (torch.autocast) only')
        if x_h and out_h:
            raise PsndError('Linear1x1: bf16 storage on one side of a projection only')
        if x_h:
            link = None
        ctx.link = None
        if link is not None and ctx.needs_input_grad[0]:
            ctx.link, link.consumer = link, True
        # relu_link: this node is the one BEFORE the ReLU (relu=True: it publishes its output) or the one AFTER it (its input is that
        # output, and a gradient for it is wanted)
        ctx.relu_out = ctx.relu_in = None
        if relu_link is not None and RELU_LINKS:
            if relu:
                ctx.relu_out = relu_link
            elif relu_link.y == (x.data_ptr(), tuple(x.shape)) and x.is_contiguous() and ctx.needs_input_grad[0]:
                ctx.relu_in, relu_link.consumer = relu_link, True
        x = x.contiguous()
        w2 = w.reshape(w.shape[0], w.shape[1]).contiguous()
        N, Cin, T = x.shape
        ld = 0
        if t_len is not None and int(t_len) != T:
            if not x_h or int(t_len) > T or int(t_len) <= 0:
                raise PsndError('Linear1x1: t_len=%s with an input %s (padded rows are a bf16 tensor\'s)' % (t_len, tuple(x.shape)))
            ld, T = T, int(t_len)
        Cout = w2.shape[0]
        if w2.shape[1] != Cin:
            raise PsndError('Linear1x1: weight %s does not fit %d input channels' % (tuple(w.shape), Cin))
        b = None if bias is None else bias.contiguous()
        if out_h and pad_h and T % 64:
            ld = (T + 63) // 64 * 64
        y = torch.empty((N, Cout, ld if (out_h and ld) else T), dtype=torch.bfloat16 if out_h else torch.float32, device=x.device)
        with on(x.device) as hip:
            hip.psnd_linear1x1_fwd_ex(x, w2, b, N, Cin, Cout, T, int(bool(relu)), int(bool(bf16)), 1 if x_h else (2 if out_h else 0), ld, y)
        ctx.relu, ctx.has_bias, ctx.wshape, ctx.bf16 = bool(relu), bias is not None, tuple(w.shape), bool(bf16)
        ctx.x_h, ctx.out_h, ctx.t_len = x_h, bool(out_h), T
        ctx.params = (w, bias)
        from . import cl
        cl.note_param_use(ctx, w, bias)
        ctx.save_for_backward(x, w2, y if relu else None)
        if ctx.relu_out is not None:
            ctx.relu_out.y = (y.data_ptr(), tuple(y.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w2, y = ctx.saved_tensors
        gy = gy.contiguous()
        if ctx.relu_out is not None and ctx.relu_out.take():
            y = None                                                    # the gradient arrives masked (ReluLink)
        T = ctx.t_len
        if gy.dtype != torch.float32 and (y is not None or ctx.x_h or not ctx.bf16):
            # a bf16 gradient that still needs this node's mask, or bf16 on both sides: outside the feed-forward pair's plan - in fp32
            gy = gy[..., :T].float()
            if y is not None:
                gy, y = gy * (y[..., :T] > 0), None
            gy = gy.contiguous()
        io_h = 1 if gy.dtype == torch.bfloat16 else (2 if ctx.x_h else 0)
        ld = (gy.shape[-1] if io_h == 1 else x.shape[-1]) if io_h else 0
        if ld == T:
            ld = 0
        xmask = x if ctx.relu_in is not None else None
        N, Cin = x.shape[0], x.shape[1]
        Cout = w2.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        dev = x.device
        addend = ctx.link.take() if ctx.link is not None else None      # the residual branch's gradient for x (ResidualLink)
        if addend is not None and (addend.shape != x.shape or addend.dtype != torch.float32 or not addend.is_contiguous()):
            raise PsndError('Linear1x1: residual gradient %s does not fit the input %s' % (tuple(addend.shape), tuple(x.shape)))
        gx = torch.empty_like(x) if need_x else None
        gw = torch.empty_like(w2) if need_w else None
        gb = torch.empty(Cout, dtype=torch.float32, device=dev) if need_b else None
        part = None
        if need_w:
            slabs = int(lib().psnd_linear1x1_wgrad_slabs(N, Cin, Cout, T))
            part = torch.empty((slabs, Cout, Cin), dtype=torch.float32, device=dev)
        # The parameter side (weight-gradient GEMM, slab sum, bias row sum: needed only by the optimizer) on the parameter stream - inside
        # the step graph a branch next to the input-gradient chain that goes on, joined at the end of the backward pass (cl.py,
        # BRANCH_PARAM_GRADS).  Only when these gradients are WRITTEN (leaf parameters without a .grad: autograd takes the tensors without
        # a launch) and nothing else shares the hardware queues with the step.
        from . import cl
        side = None
        if (need_x and (need_w or need_b) and cl.BRANCH_PARAM_GRADS and cl.AUTO_SECTIONS
                and all(q is None or (q.is_leaf and q.grad is None and cl.single_use(q)) for q in ctx.params)):
            side = cl.param_stream(dev)
            if cl.GRAD_SINK is not None:       # a reducer's bucket waits for the stream that WRITES these gradients (round 5)
                cl.GRAD_SINK.note_producer(ctx.params, side)
        with on(dev) as hip:
            if side is None:
                hip.psnd_linear1x1_bwd_ex(gy, y, x, w2, N, Cin, Cout, T, int(ctx.bf16), io_h, ld, addend, xmask, gx, gw, part, gb)
            else:
                main = torch.cuda.current_stream(dev)
                side.wait_stream(main)                          # gy is complete on the main stream
                hip.psnd_linear1x1_bwd_ex(gy, y, x, w2, N, Cin, Cout, T, int(ctx.bf16), io_h, ld, addend, xmask, gx, None, None, None)
                with torch.cuda.stream(side), on(dev) as hip_side:
                    hip_side.psnd_linear1x1_bwd_ex(gy, y, x, w2, N, Cin, Cout, T, int(ctx.bf16), io_h, ld, None, None, None, gw, part, gb)
                for t in (gy, y, x, w2, gw, part, gb):          # main-stream blocks the side stream reads / writes
                    if t is not None:
                        t.record_stream(side)
                cl._join_side_at_end_of_backward(dev, side)
        if xmask is not None and need_x:
            ctx.relu_in.masked = True
        cl.consume_param_use(ctx)
        return gx, (None if gw is None else gw.view(ctx.wshape)), gb, None, None, None, None, None, None, None


class Im2Col(torch.autograd.Function):
    """the unfolded input of a 1-d convolution, col[n][ci * k + j][t] = act(x[n][ci][(t * stride + j * dil - pad) / up]) (psnd_im2col_f32; zero
    outside the signal and between the samples of a zero-spread input), act = leaky-relu with `slope` (1.0: none); backward psnd_col2im_f32"""

    @staticmethod
    def forward(ctx, x, k, dil, pad, stride, up, To, slope):
        _need_cuda(x, 'input')
        x = x.contiguous()
        N, C, T = x.shape
        col = torch.empty((N, C * k, To), dtype=torch.float32, device=x.device)
        with on(x.device) as hip:
            hip.psnd_im2col_f32(x, N, C, T, k, dil, pad, stride, up, To, float(slope), col)
        ctx.geom = (int(k), int(dil), int(pad), int(stride), int(up), int(To), float(slope))
        ctx.save_for_backward(x if slope != 1.0 else None)
        ctx.xshape = (N, C, T)
        return col

    @staticmethod
    def backward(ctx, gcol):
        (x,) = ctx.saved_tensors
        k, dil, pad, stride, up, To, slope = ctx.geom
        N, C, T = ctx.xshape
        gcol = gcol.contiguous()
        gx = torch.empty((N, C, T), dtype=torch.float32, device=gcol.device)
        with on(gcol.device) as hip:
            hip.psnd_col2im_f32(gcol, x, N, C, T, k, dil, pad, stride, up, To, slope, gx)
        return gx, None, None, None, None, None, None, None


def conv1d_f32(x, w, bias, padding=0, dilation=1, pre_slope=1.0):
    """F.conv1d(leaky_relu(x, pre_slope), w, bias, 1, padding, dilation) in exact fp32 on the matrix cores - the precision of the reference's
    conv stack (hifi_gan.py:32-147): unfold (psnd_im2col_f32, the activation applied while gathering) + psnd_linear1x1_* (v_mfma_f32_32x32x2_f32),
    forward and both gradients.  x (N, Cin, T) fp32 HIP, w (Cout, Cin, k)."""
    Cout, Cin, k = w.shape
    T = x.shape[2]
    To = T + 2 * padding - dilation * (k - 1)
    if To <= 0:
        raise PsndError('conv1d_f32: no output samples (T=%d, k=%d, dilation=%d, padding=%d)' % (T, k, dilation, padding))
    if k == 1 and padding == 0 and pre_slope == 1.0:
        return Linear1x1.apply(x, w, bias, False, False)
    col = Im2Col.apply(x, k, dilation, padding, 1, 1, To, pre_slope)
    return Linear1x1.apply(col, w.reshape(Cout, Cin * k), bias, False, False)


def conv_transpose1d_f32(x, w, bias, stride, padding, pre_slope=1.0):
    """F.conv_transpose1d(leaky_relu(x, pre_slope), w, bias, stride, padding) in exact fp32: a convolution with the flipped taps over the
    zero-spread input (the zeros are never stored: psnd_im2col_f32 writes them into the unfolded rows), (T - 1) * stride - 2 * padding + k
    output samples (hifi_gan.py:107-110).  w (Cin, Cout, k) as nn.ConvTranspose1d keeps it."""
    Cin, Cout, k = w.shape
    T = x.shape[2]
    To = (T - 1) * stride - 2 * padding + k
    if k - 1 - padding < 0 or To <= 0:
        raise PsndError('conv_transpose1d_f32: padding %d beyond k - 1 = %d' % (padding, k - 1))
    weq = w.flip(2).permute(1, 0, 2).reshape(Cout, Cin * k)
    col = Im2Col.apply(x, k, 1, k - 1 - padding, 1, stride, To, pre_slope)
    return Linear1x1.apply(col, weq, bias, False, False)


class PosEnc(torch.autograd.Function):
    """PositionalEncoding.forward (modules.py:143-145): x * sqrt(C) + pe[..., :T] as one pass (psnd_posenc); backward g * sqrt(C)."""

    @staticmethod
    def forward(ctx, x, pe, scale):
        _need_cuda(x, 'input')
        x = x.contiguous()
        N, C, T = x.shape
        pe2 = pe.reshape(pe.shape[-2], pe.shape[-1])
        if pe2.shape[0] != C or pe2.shape[1] < T or not pe2.is_contiguous() or pe2.dtype != torch.float32 or pe2.device != x.device:
            raise PsndError('PosEnc: table %s does not cover a (%d, %d, %d) input' % (tuple(pe.shape), N, C, T))
        y = torch.empty_like(x)
        with on(x.device) as hip:
            hip.psnd_posenc(x, pe2, float(scale), N, C, T, pe2.shape[1], y)
        ctx.scale = float(scale)
        return y

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        N, C, T = g.shape
        gx = torch.empty_like(g)
        with on(g.device) as hip:
            hip.psnd_posenc(g, None, ctx.scale, N, C, T, T, gx)
        return gx, None, None


# measured, off: the two attention gradient kernels on two streams - config-4 block 2.24 -> 2.36 ms (both kernels fill the chip at 2-3 waves
# per SIMD: next to each other each runs slower than the overlap returns; tools/r04/ab_c4.sh)
ATTN_BWD_TWO_STREAMS = _sw.lab('PSND_ATTN_BWD_TWO_STREAMS', '0') == '1'


class AttentionKVQ(torch.autograd.Function):
    """MultiHeadAttention.scale_dot_att over all heads at once (modules.py:38-48, 61-79), straight from the fused projection:
    kvq (N, 3C, T) in the reference's chunk order K | V | Q, heads folded head-major -> out (N, C, T) (heads unfolded, ready for
    the output projection) and att (H*N, T_key, T_query) when `want_att`.  psnd_mha_fwd / psnd_mha_bwd: the score tensor stays
    on the chip; exact fp32 products, or (`bf16`, what the module passes under torch.autocast(bfloat16)) bf16 operands with fp32
    scores / statistics / accumulation.  mask_u8: (N, T), 1 = padding."""

    @staticmethod
    def forward(ctx, kvq, mask_u8, heads, want_att, bf16=False):
        # kvq.dtype == bfloat16 (with bf16 operands, without the attention tensor): the projection stored it that way (Linear1x1 out_h, round 6)
        # - the kernels round the operands to bf16 when they load them anyway - and the gradient goes back the same way
        kvq_h = kvq.dtype == torch.bfloat16
        if kvq_h and (not bf16 or want_att):
            raise PsndError('AttentionKVQ: a bf16-stored kvq comes with bf16 operands (torch.autocast) and without the attention tensor')
        if not (kvq_h and isinstance(kvq, torch.Tensor) and kvq.is_cuda):
            _need_cuda(kvq, 'kvq')
        kvq = kvq.contiguous()
        N, C3, T = kvq.shape
        C = C3 // 3
        dev = kvq.device
        out = torch.empty((N, C, T), dtype=torch.bfloat16 if kvq_h else torch.float32, device=dev)      # (its consumer, the output projection, rounds it to bf16 anyway)
        att = torch.empty((heads * N, T, T), dtype=torch.float32, device=dev) if want_att else None
        stats = torch.empty((heads * N, T, 2), dtype=torch.float32, device=dev)
        m = None if mask_u8 is None else mask_u8.contiguous()
        with on(dev) as hip:
            hip.psnd_mha_fwd(kvq, m, N, heads, C, T, out, att, stats, 2 if kvq_h else int(bool(bf16)))
        ctx.heads, ctx.bf16 = heads, (2 if kvq_h else int(bool(bf16)))
        ctx.set_materialize_grads(False)             # an unused `att` must not turn into an (H*N, T, T) tensor of zeros in backward
        ctx.save_for_backward(kvq, m, out, att, stats)
        if att is None:
            att = out.new_empty(0)
            ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, gout, gatt):
        kvq, m, out, att, stats = ctx.saved_tensors
        N, C3, T = kvq.shape
        C, H = C3 // 3, ctx.heads
        dev = kvq.device
        if gout is None:
            gout = torch.zeros_like(out)
        gout = gout.contiguous()
        if gatt is not None and att is None:
            gatt = None
        if gatt is not None:
            gatt = gatt.contiguous()
        if gout.dtype != out.dtype:
            gout = gout.to(out.dtype)
        delta = torch.empty((H * N, T), dtype=torch.float32, device=dev)
        gkvq = torch.empty_like(kvq)
        from . import cl
        args = (kvq, m, out, att, stats, gout, gatt, N, H, C, T, delta, gkvq, ctx.bf16)
        with on(dev) as hip:
            if ATTN_BWD_TWO_STREAMS and cl.AUTO_SECTIONS and ctx.bf16 != 2:      # (bf16 = 2 runs as a whole: its query kernel forms delta)
                # the key / value and the query gradient kernels need `delta` only and write disjoint rows of gkvq: two streams (inside
                # the step graph: two branches) behind the delta launch, joined before the projection's backward reads gkvq
                main, side = torch.cuda.current_stream(dev), cl.branch_streams(dev, 1)[0]
                hip.psnd_mha_bwd_parts(*args, 1)
                side.wait_stream(main)
                with torch.cuda.stream(side), on(dev) as hip_side:
                    hip_side.psnd_mha_bwd_parts(*args, 4)
                hip.psnd_mha_bwd_parts(*args, 2)
                main.wait_stream(side)
            else:
                hip.psnd_mha_bwd(*args)
        return gkvq, None, None, None, None


class PreEmphasisFn(torch.autograd.Function):
    """y[t] = x[t] - coef * x[t-1] with one reflect-padded sample on the left (sound.py:76-81)."""

    @staticmethod
    def forward(ctx, x, coef):
        _need_cuda(x, 'input')
        x = x.contiguous()
        T = x.shape[-1]
        N = x.numel() // max(T, 1)
        y = torch.empty_like(x)
        with on(x.device) as hip:
            hip.psnd_preemphasis_fwd(x, N, T, float(coef), y)
        ctx.coef = float(coef)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        T = gy.shape[-1]
        N = gy.numel() // max(T, 1)
        gx = torch.empty_like(gy)
        with on(gy.device) as hip:
            hip.psnd_preemphasis_bwd(gy, N, T, ctx.coef, gx)
        return gx, None


IPREEMPH_SPAN, IPREEMPH_WARM_MAX, IPREEMPH_SEQ, IPREEMPH_AUTO = (_lib.DEFINES['PSND_IPREEMPH_' + n] for n in ('SPAN', 'WARM_MAX', 'SEQ', 'AUTO'))


class InversePreEmphasisFn(torch.autograd.Function):
    """y[t] = tanh(w_ih x[t] + w_hh y[t-1]), y[-1] = 0, on (N, 1, T) fp32 - the one-unit tanh RNN of sound.py:84-99 (psnd_ipreemph_*).
    `w_ih`, `w_hh`: the RNN's (1, 1) parameters on the input's device; the kernels read them there, so no host copy can be stale.
    `warm`: IPREEMPH_AUTO (the kernel applies the warm-up rule to w_hh), IPREEMPH_SEQ, or a warm-up length (psnd.h)."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, warm=IPREEMPH_AUTO):
        _need_cuda(x, 'input')
        for w, name in ((w_ih, 'weight_ih'), (w_hh, 'weight_hh')):
            _need_cuda(w, name)
            if w.numel() != 1 or w.device != x.device:
                raise _lib.PsndError('InversePreEmphasis: %s must hold one element on %s, got %s on %s'
                                     % (name, x.device, tuple(w.shape), w.device))
        x = x.contiguous()
        T = x.shape[-1]
        N = x.numel() // max(T, 1)
        y = torch.empty_like(x)
        with on(x.device) as hip:
            hip.psnd_ipreemph_fwd(x, N, T, w_ih, w_hh, int(warm), y)
        ctx.save_for_backward(x, y, w_ih, w_hh)
        ctx.warm = int(warm)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, w_ih, w_hh = ctx.saved_tensors
        gy = gy.contiguous()
        T = x.shape[-1]
        N = x.numel() // max(T, 1)
        gx = torch.empty_like(x)
        partial = torch.empty(2 * 256 * max(N, 1) * max((T + IPREEMPH_SPAN - 1) // IPREEMPH_SPAN, 1), dtype=torch.float64, device=x.device)
        gw = torch.empty(2, dtype=torch.float32, device=x.device)
        with on(x.device) as hip:
            hip.psnd_ipreemph_bwd(gy, y, x, N, T, w_ih, w_hh, ctx.warm, gx, partial, gw)
        need = ctx.needs_input_grad
        return (gx if need[0] else None, gw[0].reshape(w_ih.shape) if need[1] else None, gw[1].reshape(w_hh.shape) if need[2] else None, None)


LFILTER_SPAN, LFILTER_PARALLEL, LFILTER_SEQ = (_lib.DEFINES['PSND_LFILTER_' + n] for n in ('SPAN', 'PARALLEL', 'SEQ'))


def lfilter_section(b, a):
    """(b0, b1, b2, a1, a2): the coefficients of one section of order <= 2 divided by a[0] in float64, missing ones zero"""
    b, a = np.asarray(b, dtype=np.float64).ravel().tolist(), np.asarray(a, dtype=np.float64).ravel().tolist()
    if not 1 <= len(b) <= 3 or not 1 <= len(a) <= 3:
        raise _lib.PsndError('lfilter: %d numerator and %d denominator coefficients - sections of order <= 2 (at most three each) are covered'
                             % (len(b), len(a)))
    if a[0] == 0.0:
        raise ValueError('lfilter: a[0] must not be zero')
    b, a = [v / a[0] for v in b] + [0.0] * (3 - len(b)), [v / a[0] for v in a] + [0.0] * (3 - len(a))
    return b[0], b[1], b[2], a[1], a[2]


def lfilter_instance(b, a):
    """the instance of psnd_lfilter for this filter (the rule of include/psnd.h, host numbers only): LFILTER_PARALLEL while every entry of
    M^8192, M = [[-a1, 1], [-a2, 0]], is finite - every pole inside or on the unit circle, and outside it as far as the power stays
    finite; LFILTER_SEQ otherwise and for coefficients that are not finite."""
    sec = lfilter_section(b, a)
    if not all(math.isfinite(v) for v in sec):
        return LFILTER_SEQ
    m = (-sec[3], 1.0, -sec[4], 0.0)
    for _ in range(13):                                  # 2^13 = 8192, by squaring as the library does
        m = (m[0] * m[0] + m[1] * m[2], m[0] * m[1] + m[1] * m[3], m[2] * m[0] + m[3] * m[2], m[2] * m[1] + m[3] * m[3])
    return LFILTER_PARALLEL if all(math.isfinite(v) for v in m) else LFILTER_SEQ


def _lfilter_rows(x, sec, reverse, instance):
    if x.dim() == 0:
        raise _lib.PsndError('lfilter: the input needs a time axis')
    if not x.is_cuda:                                    # the reference's own path: scipy on the host, in float64
        from scipy.signal import lfilter as host_lfilter
        if not x.is_floating_point():
            raise _lib.PsndError('lfilter: floating input expected, got %s' % x.dtype)
        if x.numel() == 0:
            return torch.empty_like(x)
        v = x.detach().to(torch.float64).numpy()
        v = v[..., ::-1] if reverse else v
        y = host_lfilter(sec[:3], (1.0,) + sec[3:], v, axis=-1)
        return torch.from_numpy(np.ascontiguousarray(y[..., ::-1] if reverse else y)).to(x.dtype)
    if x.dtype == torch.float64:
        raise _lib.PsndError('lfilter: no float64 instance on HIP tensors (a round trip through float32 would silently lose the precision '
                             'asked for): filter a float32 tensor, or a CPU tensor in float64')
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.PsndError('lfilter: floating input expected, got %s' % x.dtype)
    xf = x.detach().contiguous().float()
    T = xf.shape[-1]
    N = xf.numel() // max(T, 1)
    y = torch.empty_like(xf)
    carry = None
    if instance == LFILTER_PARALLEL:
        carry = torch.empty(2 * N * int(lib().psnd_lfilter_spans(T)), dtype=torch.float64, device=x.device)
    with on(x.device) as hip:
        hip.psnd_lfilter(xf, N, T, *sec, int(bool(reverse)), int(instance), carry, y)
    return y.to(x.dtype)


class LFilterFn(torch.autograd.Function):
    """one filter section on the last axis; the gradient is the same Function mirrored in time, so nothing is saved and it composes for a
    second derivative"""

    @staticmethod
    def forward(ctx, x, sec, reverse, instance):
        ctx.sec, ctx.reverse, ctx.instance = sec, reverse, instance
        return _lfilter_rows(x, sec, reverse, instance)

    @staticmethod
    def backward(ctx, gy):
        return LFilterFn.apply(gy, ctx.sec, not ctx.reverse, ctx.instance), None, None, None


def lfilter(x, b, a, reverse=False, instance=None):
    """scipy.signal.lfilter(b, a, x) with zero initial state along the last axis of a tensor of any shape (..., T), for a section of order
    <= 2: y[t] = (b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2]) / a0.  `reverse`: the same filter mirrored in time (the adjoint).

    HIP tensors run psnd_lfilter (float32; float16 / bfloat16 are cast in and out; float64 raises), CPU tensors scipy in float64 - the one
    entry of this module with a host path, because the reference's own implementation is that scipy call.  Differentiable in x on both
    devices; `b` and `a` are plain numbers and carry no gradient.  `instance`: LFILTER_PARALLEL or LFILTER_SEQ instead of the rule of
    `lfilter_instance` (HIP tensors only)."""
    sec = lfilter_section(b, a)
    if instance is None:
        instance = lfilter_instance(b, a)
    elif instance not in (LFILTER_PARALLEL, LFILTER_SEQ):
        raise _lib.PsndError('lfilter: instance=%r' % (instance,))
    return LFilterFn.apply(x, sec, bool(reverse), instance)


RESAMPLE_TILE, RESAMPLE_MAX_TAPS = _lib.DEFINES['PSND_RESAMPLE_TILE'], _lib.DEFINES['PSND_RESAMPLE_MAX_TAPS']


def resample_ratio(orig_sr, new_sr):
    """(up, down) of a conversion from orig_sr to new_sr Hz, divided by their gcd.  Integer rates only: anything else, and a rate <= 0,
    raises ValueError."""
    rates = []
    for name, v in (('orig_sr', orig_sr), ('new_sr', new_sr)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError('resample: %s=%r - integer sample rates only' % (name, v))
        if v <= 0:
            raise ValueError('resample: %s=%r must be positive' % (name, v))
        rates.append(int(v))
    g = math.gcd(*rates)
    return rates[1] // g, rates[0] // g


def _resample_factors(up, down):
    for name, v in (('up', up), ('down', down)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0:
            raise ValueError('resample: %s=%r - a positive integer factor' % (name, v))
    g = math.gcd(int(up), int(down))
    return int(up) // g, int(down) // g


def resample_taps(up, down):
    """the filter of scipy.signal.resample_poly(x, up, down) in float64, gain included: P = 10 max(up, down) for the reduced factors and
    h = firwin(2P + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up.  Equal factors have no filter to design (scipy returns a copy):
    the one tap 1."""
    from scipy.signal import firwin
    up, down = _resample_factors(up, down)
    big = max(up, down)
    if big == 1:
        return np.ones(1)
    return firwin(2 * 10 * big + 1, 1.0 / big, window=('kaiser', 5.0)) * up


class ResampleTaps:
    """the filter of one conversion: `h`, the float64 values that are applied (gain included), `window`, what scipy.signal.resample_poly
    takes as `window=` for them, and the float32 copy of h per device, made on first use and kept - a later call copies nothing from the
    host and can be captured into a graph."""

    def __init__(self, h, window):
        self.h = np.ascontiguousarray(h, dtype=np.float64)
        self.h.setflags(write=False)
        self.window = window
        self._on = {}

    def on(self, device):
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = torch.from_numpy(self.h.astype(np.float32)).to(device)
        return t


_RESAMPLE_TAPS = {}


def resample_plan(up, down, taps=None):
    """the cached ResampleTaps of reduced factors (up, down): the default filter, or `taps` as scipy takes an array for `window=` - an
    odd-length prototype of unit gain that is applied times `up`"""
    up, down = _resample_factors(up, down)
    if taps is None:
        key = (up, down, None)
    else:
        w = np.asarray(taps, dtype=np.float64)
        if w.ndim != 1 or w.size % 2 == 0:
            raise ValueError('resample: taps must be a sequence of odd length, got shape %s' % (w.shape,))
        key = (up, down, w.tobytes())
    plan = _RESAMPLE_TAPS.get(key)
    if plan is None:
        plan = _RESAMPLE_TAPS[key] = ResampleTaps(resample_taps(up, down), ('kaiser', 5.0)) if taps is None else ResampleTaps(w * up, w.copy())
    return plan


def _resample_host(v, up, down, plan, flip, out_len):
    """the definition on a float64 array (..., T): scipy.signal.resample_poly where that is the call, else scipy.signal.upfirdn with the
    zeros in front of the filter that put output 0 on a multiple of `down`, as resample_poly does inside"""
    from scipy import signal
    T = v.shape[-1]
    if not flip and out_len == -(-T * up // down) and T > 0:
        return signal.resample_poly(v, up, down, axis=-1, window=plan.window if isinstance(plan.window, tuple) else plan.window.copy())
    out = np.zeros(v.shape[:-1] + (out_len,), dtype=np.float64)
    if T == 0 or out_len == 0:
        return out
    g = plan.h[::-1] if flip else plan.h
    P = g.size // 2
    pre = down - P % down
    skip = (P + pre) // down
    full = signal.upfirdn(np.concatenate((np.zeros(pre), g)), v, up, down, axis=-1)[..., skip:skip + out_len]
    out[..., :full.shape[-1]] = full
    return out


def _resample_rows(x, up, down, plan, flip, out_len, device_taps):
    T = x.shape[-1]
    if not x.is_cuda:
        if x.numel() == 0:
            return x.new_zeros(x.shape[:-1] + (out_len,))
        y = _resample_host(x.detach().to(torch.float64).numpy(), up, down, plan, flip, out_len)
        return torch.from_numpy(np.ascontiguousarray(y)).to(x.dtype)
    taps = plan.h.size
    h = plan.on(x.device) if device_taps is None else device_taps
    if h.device != x.device or h.dtype != torch.float32 or h.numel() != taps or not h.is_contiguous():
        raise _lib.PsndError('resample: the device taps must be %d contiguous float32 values on %s, got %s %s on %s'
                             % (taps, x.device, tuple(h.shape), h.dtype, h.device))
    xf = x.detach().contiguous().float()
    N = math.prod(xf.shape[:-1])                         # rows, also where T == 0: those write zeros
    y = torch.empty(xf.shape[:-1] + (out_len,), dtype=torch.float32, device=x.device)
    with on(x.device) as hip:
        hip.psnd_resample(xf, N, T, h, taps, up, down, int(bool(flip)), y, out_len)
    return y.to(x.dtype)


class ResampleFn(torch.autograd.Function):
    """y[m] = sum_i x[i] g[m down - i up + P] on the last axis (include/psnd.h); the gradient is the same Function with up and down
    exchanged, the taps reversed and the input's length as out_len, so nothing is saved and it composes for a second derivative"""

    @staticmethod
    def forward(ctx, x, up, down, taps, flip, out_len, device_taps):
        ctx.args = (up, down, taps, flip, x.shape[-1], device_taps)
        return _resample_rows(x, up, down, taps, flip, out_len, device_taps)

    @staticmethod
    def backward(ctx, gy):
        up, down, taps, flip, T, device_taps = ctx.args
        return ResampleFn.apply(gy, down, up, taps, not flip, T, device_taps), None, None, None, None, None, None


def resample_poly(x, up, down, taps=None, device_taps=None):
    """scipy.signal.resample_poly(x, up, down) with zero padding along the last axis of a tensor of any shape (..., T): the result has
    ceil(T up / down) samples (up, down reduced by their gcd; equal factors return a copy).  `taps`: an odd-length sequence instead of the
    default Kaiser design, as scipy takes an array for `window=` (unit gain; the filter applied is taps * up).

    HIP tensors run psnd_resample (float32; float16 / bfloat16 are cast in and out; float64 raises); the float32 taps live on the device,
    cached per (up, down, taps, device), or are `device_taps` where the caller keeps them (models.sound.Resample's buffer).  Taps beyond
    RESAMPLE_MAX_TAPS raise: no host path for a HIP tensor.  CPU tensors go through scipy in float64.  Differentiable in x on both
    devices, any number of times."""
    if not isinstance(x, torch.Tensor):
        raise _lib.PsndError('resample: a tensor is expected, got %s' % type(x).__name__)
    if x.dim() == 0:
        raise _lib.PsndError('resample: the input needs a time axis')
    if not x.is_floating_point():
        raise _lib.PsndError('resample: floating input expected, got %s' % x.dtype)
    up, down = _resample_factors(up, down)
    plan = resample_plan(up, down, taps)
    if up == down:
        return x.clone()
    if x.is_cuda:
        if x.dtype == torch.float64:
            raise _lib.PsndError('resample: no float64 instance on HIP tensors (a round trip through float32 would silently lose the '
                                 'precision asked for): resample a float32 tensor, or a CPU tensor in float64')
        if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise _lib.PsndError('resample: floating input expected, got %s' % x.dtype)
        if plan.h.size > RESAMPLE_MAX_TAPS:
            raise _lib.PsndError('resample: %d taps for the ratio %d / %d, the kernel holds at most RESAMPLE_MAX_TAPS = %d (no host path for '
                                 'a HIP tensor)' % (plan.h.size, up, down, RESAMPLE_MAX_TAPS))
    return ResampleFn.apply(x, up, down, plan, False, -(-x.shape[-1] * up // down), device_taps)


SILENCE_BLOCK = _lib.DEFINES['PSND_SILENCE_BLOCK']


def silence_theta(min_silence_len, silence_thresh):
    """L 10^(dB/10) in float64: the bound on a window's energy that is the reference's rms <= 10^(dB/20).  -inf dB gives 0."""
    db = float(silence_thresh)
    if math.isnan(db):
        raise ValueError('silence: silence_thresh is NaN')
    try:
        return float(min_silence_len) * 10.0 ** (db / 10.0)
    except OverflowError:
        return _INF


def silence_cap(T, L):
    """psnd_silence_cap: floor((T - L) / (L + 1)) + 1 ranges always suffice for a row of T samples, 0 for T < L"""
    return 0 if L < 1 or T < L else (T - L) // (L + 1) + 1


def silence_starts(T, L, s):
    """psnd_silence_starts: the window starts 0, s, 2s, ... <= T - L and T - L itself"""
    if T < L or T <= 0:
        return np.zeros(0, dtype=np.int64)
    i = np.arange(0, T - L + 1, s, dtype=np.int64)
    return i if (T - L) % s == 0 else np.append(i, np.int64(T - L))


def silence_energies(x, L, starts):
    """(E, bad) of the windows [i, i + L) of one row, i in `starts`: the float64 energy with non-finite samples counted as 0, and the number
    of non-finite samples.  The decomposition of psnd_silence.hip: prefix sums restarted every SILENCE_BLOCK samples, a window = tail of its
    first block + whole blocks + head of its last block, so that a quiet window behind a loud passage keeps its digits."""
    T, B = x.shape[0], SILENCE_BLOCK
    if starts.size * L <= T:                                            # few windows (a wide step): each summed on its own, pairwise
        w = np.asarray(x)[starts[:, None] + np.arange(L)].astype(np.float64)
        fin = np.isfinite(w)
        return (np.where(fin, w, 0.0) ** 2).sum(axis=1), (~fin).sum(axis=1)
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x)
    nb = -(-T // B)
    sq = np.zeros(nb * B)
    sq[:T] = np.where(fin, x, 0.0) ** 2
    P = np.cumsum(sq.reshape(nb, B), axis=1).reshape(-1)                # inclusive, restarted per block
    cnt = np.concatenate(([0], np.cumsum(~fin, dtype=np.int64)))       # integers: one row-long prefix is exact
    e = starts + L - 1
    b0, b1 = starts // B, e // B
    before = np.where(starts % B == 0, 0.0, P[starts - 1])
    same = b0 == b1
    E = np.where(same, P[e] - before, P[b0 * B + B - 1] - before)
    for k in range(1, L // B + 2):                                      # whole blocks between, first to last
        b = b0 + k
        E = E + np.where(b < b1, P[np.minimum(b, nb - 1) * B + B - 1], 0.0)
    E = E + np.where(same, 0.0, P[e])
    return E, cnt[starts + L] - cnt[starts]


def silence_merge(k, L, s):
    """silent starts `k` (ascending) -> (R, 2) ranges by the rule of include/psnd.h: k opens a range iff it is the first, or k != p + s and
    k > p + L for the silent start p before it; a range is [first start, last start + L]"""
    if k.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    head = np.ones(k.size, dtype=bool)
    head[1:] = (k[1:] != k[:-1] + s) & (k[1:] > k[:-1] + L)
    first = np.flatnonzero(head)
    last = np.append(first[1:] - 1, k.size - 1)
    return np.stack((k[first], k[last] + L), axis=1).astype(np.int64)


def silence_ranges_host(x, L, s, theta):
    """the definition on one row of numpy samples: (R, 2) int64"""
    x = np.asarray(x).reshape(-1)
    starts = silence_starts(x.shape[0], L, s)
    if starts.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    E, bad = silence_energies(x, L, starts)
    return silence_merge(starts[(bad == 0) & (E <= theta)], L, s)


def silence_params(min_silence_len, seek_step):
    for name, v in (('min_silence_len', min_silence_len), ('seek_step', seek_step)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError('silence: %s=%r - a count of samples, at least 1' % (name, v))
    return int(min_silence_len), int(seek_step)


def silence_ranges(wav, min_silence_len, silence_thresh, seek_step=1, lengths=None):
    """the silent ranges of every row of `wav` (..., T) by the definition of include/psnd.h (the reference's utils/silence.py detect_silence):
    (count (N,) int32, ranges (N, cap, 2) int64) on wav's device, N = the product of the leading shape, cap = silence_cap(T, L); row n
    has count[n] ranges [start, end], the entries behind them are -1.  `lengths`: per-row valid lengths (N,), clamped to [0, T].

    HIP tensors run psnd_silence_ranges (float32; float16 / bfloat16 are cast; float64 raises) with no host synchronisation - the call can
    be captured; `lengths` is then an int64 tensor on the same device (anything else is copied there).  CPU tensors go through the host
    restatement above in float64.  No autograd: the outputs are integers."""
    if not isinstance(wav, torch.Tensor):
        raise _lib.PsndError('silence: a tensor is expected, got %s' % type(wav).__name__)
    if wav.dim() == 0:
        raise _lib.PsndError('silence: the input needs a time axis')
    if not wav.is_floating_point():
        raise _lib.PsndError('silence: floating input expected, got %s' % wav.dtype)
    L, s = silence_params(min_silence_len, seek_step)
    theta = silence_theta(L, silence_thresh)
    T = wav.shape[-1]
    N = math.prod(wav.shape[:-1])
    cap = silence_cap(T, L)
    if lengths is not None:
        lengths = torch.as_tensor(lengths)
        if lengths.is_floating_point() or lengths.numel() != N:
            raise _lib.PsndError('silence: lengths must be %d integers, got %s %s' % (N, tuple(lengths.shape), lengths.dtype))
    if not wav.is_cuda:
        rows = wav.detach().reshape(N, T).to(torch.float64).numpy()
        lens = [T] * N if lengths is None else [min(max(int(v), 0), T) for v in lengths.reshape(-1).tolist()]
        count = np.zeros(N, dtype=np.int32)
        ranges = np.full((N, cap, 2), -1, dtype=np.int64)
        for n in range(N):
            r = silence_ranges_host(rows[n, :lens[n]], L, s, theta)
            count[n] = r.shape[0]
            ranges[n, :r.shape[0]] = r
        return torch.from_numpy(count), torch.from_numpy(ranges)
    if wav.dtype == torch.float64:
        raise _lib.PsndError('silence: no float64 instance on HIP tensors (a round trip through float32 would silently change which windows '
                             'pass the threshold): pass a float32 tensor, or a CPU tensor in float64')
    if wav.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.PsndError('silence: floating input expected, got %s' % wav.dtype)
    xf = wav.detach().reshape(N, T).float()
    if N * T > 0 and (xf.stride(-1) != 1 or (N > 1 and xf.stride(0) != T)):
        xf = xf.contiguous()
    if lengths is not None:
        lengths = lengths.reshape(-1).to(device=wav.device, dtype=torch.int64).contiguous()
    if N * T == 0:                                       # nothing to launch: rows without samples have no ranges
        return torch.zeros(N, dtype=torch.int32, device=wav.device), torch.empty((N, 0, 2), dtype=torch.int64, device=wav.device)
    count = torch.empty(N, dtype=torch.int32, device=wav.device)
    ranges = torch.empty((N, cap, 2), dtype=torch.int64, device=wav.device)
    nbytes = int(lib().psnd_silence_scratch_bytes(N, T, L, s))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=wav.device) if nbytes else None
    with on(wav.device) as hip:
        hip.psnd_silence_ranges(xf, N, T, lengths, L, s, theta, scratch, count, ranges, cap)
    return count, ranges


# ---- loudness (include/psnd.h: ITU-R BS.1770-4 / EBU R128 integrated loudness), plain levels, gain ----------------------------------------
LOUDNESS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)        # the absolute gate as a block energy
LOUDNESS_WEIGHTS = (1.0, 1.0, 1.0, 1.41, 1.41)
LEVEL_KINDS = ('rms', 'peak')


def k_weighting(sr):
    """((b, a) of the shelf, (b, a) of the high-pass) of the K-weighting at `sr` Hz in float64, a[0] = 1: the formulas of include/psnd.h,
    which give the table of BS.1770 at 48 kHz"""
    sr = float(sr)
    if not (math.isfinite(sr) and sr > 0.0):
        raise ValueError('loudness: sr=%r must be positive' % (sr,))
    K = math.tan(math.pi * 1681.974450955533 / sr)
    Q = 0.7071752369554196
    Vh = 10.0 ** (3.999843853973347 / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = ([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0],
             [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    K = math.tan(math.pi * 38.13547087602444 / sr)
    Q = 0.5003270373238773
    a0 = 1.0 + K / Q + K * K
    return shelf, ([1.0, -2.0, 1.0], [1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def loudness_block(sr):
    """(B, H): the block of 400 ms and the hop of a quarter of it in samples, B = round(0.4 sr), H = B // 4"""
    B = int(math.floor(0.4 * float(sr) + 0.5))
    if B < 4:
        raise ValueError('loudness: sr=%r is too low for a block of 400 ms' % (sr,))
    return B, B // 4


def loudness_blocks(T, B, H):
    """psnd_loudness_blocks: the complete blocks of a row of T samples"""
    return 0 if B < 1 or H < 1 or T < B else (T - B) // H + 1


def loudness_span():
    """psnd_loudness_span: the samples per workgroup, the one size the kernel's seams depend on"""
    return int(lib().psnd_loudness_span())


def _programmes(shape, channels, who):
    """(leading shape, N, C, T) of an input (..., T) of mono rows, or (..., C, T) with channels=C"""
    if len(shape) == 0:
        raise _lib.PsndError('%s: the input needs a time axis' % who)
    if channels is None:
        C, lead = 1, tuple(shape[:-1])
    else:
        if isinstance(channels, bool) or not isinstance(channels, (int, np.integer)) or channels < 1:
            raise ValueError('%s: channels=%r - a count, at least 1' % (who, channels))
        C = int(channels)
        if len(shape) < 2 or shape[-2] != C:
            raise _lib.PsndError('%s: channels=%d expects an input (..., %d, T), got %s' % (who, C, C, tuple(shape)))
        lead = tuple(shape[:-2])
    return lead, math.prod(lead), C, int(shape[-1])


def _loudness_weights(C, weights):
    if weights is None:
        if C > len(LOUDNESS_WEIGHTS):
            raise _lib.PsndError('loudness: %d channels need explicit weights (the default covers %d)' % (C, len(LOUDNESS_WEIGHTS)))
        return list(LOUDNESS_WEIGHTS[:C])
    w = np.asarray(weights, dtype=np.float64).reshape(-1).tolist()
    if len(w) != C or not all(math.isfinite(v) for v in w):
        raise _lib.PsndError('loudness: weights=%r - %d finite numbers' % (weights, C))
    return w


def _host_lengths(lengths, N, T, who):
    if lengths is None:
        return [T] * N
    v = np.asarray(lengths.detach().cpu() if isinstance(lengths, torch.Tensor) else lengths)
    if v.dtype.kind not in 'iu' or v.size != N:
        raise _lib.PsndError('%s: lengths must be %d integers, got %s %s' % (who, N, v.shape, v.dtype))
    return [min(max(int(k), 0), T) for k in v.reshape(-1).tolist()]


def _device_lengths(lengths, N, device, who):
    if lengths is None:
        return None
    lengths = torch.as_tensor(lengths)
    if lengths.is_floating_point() or lengths.numel() != N:
        raise _lib.PsndError('%s: lengths must be %d integers, got %s %s' % (who, N, tuple(lengths.shape), lengths.dtype))
    return lengths.reshape(-1).to(device=device, dtype=torch.int64).contiguous()


def loudness_gate(z):
    """the two gates of BS.1770 on the block energies z (float64): L in LUFS as a Python float, -inf where no block passes the absolute gate"""
    z = np.asarray(z, dtype=np.float64)
    za = z[z > LOUDNESS_GATE]
    if za.size == 0:
        return -_INF
    zg = za[za > 0.1 * za.mean()]
    return -0.691 + 10.0 * math.log10(zg.mean())


def gain_of_level(level, target):
    """float32 gains 10^((target - level) / 20) of float32 levels in dB; exactly 1 where the level is not finite"""
    level = np.asarray(level, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        g = np.power(10.0, (float(target) - level.astype(np.float64)) / 20.0).astype(np.float32)
    return np.where(np.isfinite(level), g, np.float32(1.0)).astype(np.float32)


def loudness_host(x, sr, lengths=None, channels=None, weights=None, return_blocks=False):
    """the definition of include/psnd.h in float64 numpy on an array (..., T), or (..., C, T) with channels=C: float32 LUFS of the leading
    shape, and with return_blocks the block energies z[j] (leading shape, Jmax) in float32, 0 behind a row's blocks.  A programme that
    holds a non-finite sample reads NaN."""
    from scipy.signal import lfilter as host_lfilter
    x = np.asarray(x)
    lead, N, C, T = _programmes(x.shape, channels, 'loudness')
    G = np.asarray(_loudness_weights(C, weights), dtype=np.float64)
    (b1, a1), (b2, a2) = k_weighting(sr)
    B, H = loudness_block(sr)
    lens = _host_lengths(lengths, N, T, 'loudness')
    Jmax = loudness_blocks(T, B, H)
    rows = x.reshape(N, C, T)
    lufs = np.full(N, -np.inf, dtype=np.float32)
    blocks = np.zeros((N, Jmax), dtype=np.float32)
    for n in range(N):
        v = rows[n, :, :lens[n]].astype(np.float64)
        J = loudness_blocks(lens[n], B, H)
        if not np.isfinite(v).all():
            lufs[n], blocks[n, :J] = np.nan, np.nan
            continue
        if J == 0:
            continue
        y = host_lfilter(b2, a2, host_lfilter(b1, a1, v, axis=-1), axis=-1)
        e = np.lib.stride_tricks.sliding_window_view(y * y, B, axis=-1)[:, ::H].sum(axis=-1)           # (C, J)
        z = (G[:, None] * e).sum(axis=0) / B
        blocks[n, :J] = z
        lufs[n] = loudness_gate(z)
    lufs = lufs.reshape(lead)
    return (lufs, blocks.reshape(lead + (Jmax,))) if return_blocks else lufs


def level_host(x, kind, lengths=None, channels=None):
    """float32 rms_db = 10 log10(mean x^2) or peak_db = 20 log10(max |x|) per programme in float64 numpy; -inf for silence or no samples,
    NaN where a sample is not finite"""
    if kind not in LEVEL_KINDS:
        raise ValueError("level: kind=%r - 'rms' or 'peak'" % (kind,))
    x = np.asarray(x)
    lead, N, C, T = _programmes(x.shape, channels, 'level')
    lens = _host_lengths(lengths, N, T, 'level')
    rows = x.reshape(N, C, T)
    out = np.full(N, -np.inf, dtype=np.float32)
    for n in range(N):
        v = rows[n, :, :lens[n]].astype(np.float64)
        if not np.isfinite(v).all():
            out[n] = np.nan
        elif v.size and np.abs(v).max() > 0.0:
            out[n] = 10.0 * math.log10(float((v * v).sum()) / v.size) if kind == 'rms' else 20.0 * math.log10(float(np.abs(v).max()))
    return out.reshape(lead)


def apply_gain_host(x, gain, lengths=None, channels=None):
    """float32 x gain[programme] before the programme's length, x behind it (numpy)"""
    x = np.asarray(x)
    lead, N, C, T = _programmes(x.shape, channels, 'apply_gain')
    g = np.asarray(gain, dtype=np.float32).reshape(-1)
    if g.size != N:
        raise _lib.PsndError('apply_gain: %d gains for %d programmes' % (g.size, N))
    lens = np.asarray(_host_lengths(lengths, N, T, 'apply_gain'), dtype=np.int64)
    xf = x.reshape(N, C, T).astype(np.float32)
    live = np.arange(T)[None, None, :] < lens[:, None, None]
    return np.where(live, xf * g[:, None, None], xf).astype(np.float32).reshape(x.shape)


def _meter_rows(wav, channels, who):
    """a HIP tensor as (N C, T) float32 rows the kernels can walk (any 4-byte start, unit stride in time, rows T apart), with its geometry"""
    if not isinstance(wav, torch.Tensor) or not wav.is_cuda:
        raise _lib.PsndError('%s: a HIP tensor is expected here (CPU tensors and numpy arrays take the host path of the public function)' % who)
    lead, N, C, T = _programmes(wav.shape, channels, who)
    if not wav.is_floating_point():
        raise _lib.PsndError('%s: floating input expected, got %s' % (who, wav.dtype))
    xf = wav.detach().reshape(N * C, T)
    if xf.dtype != torch.float32:
        xf = xf.float()
    if N * C * T > 0 and (xf.stride(-1) != 1 or (N * C > 1 and xf.stride(0) != T)):
        xf = xf.contiguous()
    return xf, lead, N, C, T


def loudness_gain(wav, sr, target=-23.0, lengths=None, channels=None, weights=None, return_blocks=False):
    """one call of psnd_loudness on a HIP tensor: (lufs, gain, blocks or None) - float32 LUFS and the gains 10^((target - lufs) / 20), both of
    the leading shape (gain 1 where the loudness is not finite), and the block energies (leading shape, Jmax)"""
    xf, lead, N, C, T = _meter_rows(wav, channels, 'loudness')
    G = _loudness_weights(C, weights)
    (b1, a1), (b2, a2) = k_weighting(sr)
    B, H = loudness_block(sr)
    lengths = _device_lengths(lengths, N, wav.device, 'loudness')
    Jmax = loudness_blocks(T, B, H)
    dev = wav.device
    if N * T == 0:                                       # nothing to launch: no blocks, no loudness
        blocks = torch.zeros(lead + (Jmax,), dtype=torch.float32, device=dev) if return_blocks else None
        return torch.full(lead, -_INF, dtype=torch.float32, device=dev), torch.ones(lead, dtype=torch.float32, device=dev), blocks
    lufs = torch.empty(N, dtype=torch.float32, device=dev)
    gain = torch.empty(N, dtype=torch.float32, device=dev)
    blocks = torch.empty((N, Jmax), dtype=torch.float32, device=dev) if return_blocks else None
    scratch = torch.empty(int(lib().psnd_loudness_scratch_bytes(N, C, T, B, H)), dtype=torch.uint8, device=dev)
    with on(dev) as hip:
        hip.psnd_loudness(xf, N, C, T, lengths, b1[0], b1[1], b1[2], a1[1], a1[2], b2[0], b2[1], b2[2], a2[1], a2[2], B, H,
                          (ctypes.c_double * C)(*G), float(target), scratch, lufs, blocks, gain)
    return lufs.reshape(lead), gain.reshape(lead), (blocks.reshape(lead + (Jmax,)) if return_blocks else None)


def loudness(wav, sr, lengths=None, channels=None, weights=None, return_blocks=False):
    """integrated loudness in LUFS (ITU-R BS.1770-4 / EBU R128, the definition of include/psnd.h) of every programme of `wav`: float32 of
    the leading shape.  `wav` is (..., T), every row a mono programme, or (..., C, T) with channels=C; `weights`: C channel weights
    (default 1, 1, 1, 1.41, 1.41 for C <= 5); `lengths`: per-programme valid lengths, clamped to [0, T].  return_blocks: also the block
    energies z[j] (leading shape, Jmax) float32 - the momentary curve is -0.691 + 10 log10 z.  -inf for a programme that is silent or
    shorter than a block of 400 ms, NaN for one that holds a non-finite sample.

    HIP tensors run psnd_loudness (float32 samples; other float dtypes are cast) with no host synchronisation - the call can be captured;
    CPU tensors and numpy arrays go through `loudness_host` in float64.  No autograd: the meter is not differentiated."""
    if isinstance(wav, torch.Tensor) and wav.is_cuda:
        lufs, _, blocks = loudness_gain(wav, sr, -23.0, lengths, channels, weights, return_blocks)
        return (lufs, blocks) if return_blocks else lufs
    tensor = isinstance(wav, torch.Tensor)
    x = wav.detach().numpy() if tensor and wav.dtype != torch.bfloat16 else (wav.detach().float().numpy() if tensor else wav)
    r = loudness_host(x, sr, lengths, channels, weights, return_blocks)
    if not tensor:
        return r
    return (torch.from_numpy(r[0].copy()), torch.from_numpy(r[1].copy())) if return_blocks else torch.from_numpy(np.array(r))


def level_gain(wav, kind, target=0.0, lengths=None, channels=None):
    """one call of psnd_row_level on a HIP tensor: (level in dB, gain 10^((target - level) / 20)), float32 of the leading shape"""
    if kind not in LEVEL_KINDS:
        raise ValueError("level: kind=%r - 'rms' or 'peak'" % (kind,))
    xf, lead, N, C, T = _meter_rows(wav, channels, 'level')
    lengths = _device_lengths(lengths, N, wav.device, 'level')
    db = torch.empty(N, dtype=torch.float32, device=wav.device)
    gain = torch.empty(N, dtype=torch.float32, device=wav.device)
    if N > 0:
        with on(wav.device) as hip:
            hip.psnd_row_level(xf, N, C, T, lengths, int(kind == 'peak'), float(target), db if kind == 'rms' else None,
                               db if kind == 'peak' else None, gain)
    return db.reshape(lead), gain.reshape(lead)


def level(wav, kind, lengths=None, channels=None):
    """the plain level of every programme of `wav` in dB re full scale, float32 of the leading shape: kind 'rms' 10 log10(mean x^2) over the
    programme's channels and samples, 'peak' 20 log10(max |x|) (the sample peak, not the oversampled true peak).  -inf for silence, NaN
    where a sample is not finite.  Shapes, `lengths`, `channels` and devices as `loudness`; HIP tensors run psnd_row_level."""
    if isinstance(wav, torch.Tensor) and wav.is_cuda:
        return level_gain(wav, kind, 0.0, lengths, channels)[0]
    tensor = isinstance(wav, torch.Tensor)
    r = level_host(wav.detach().float().numpy() if tensor and wav.dtype == torch.bfloat16 else (wav.detach().numpy() if tensor else wav),
                   kind, lengths, channels)
    return torch.from_numpy(np.array(r)) if tensor else r


def apply_gain(wav, gain, lengths=None, channels=None, out=None):
    """`wav` with every programme multiplied by its entry of `gain` (one per programme, read from device memory on a HIP tensor: no host
    round trip); samples behind `lengths` are copied unchanged.  Comes back in wav's dtype.  out: a float32 HIP tensor of wav's shape to
    write into, `wav` itself for in place (float32, contiguous rows).  CPU tensors and numpy arrays go through numpy."""
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda):
        if out is not None:
            raise _lib.PsndError('apply_gain: out= is for HIP tensors')
        tensor = isinstance(wav, torch.Tensor)
        g = gain.detach().cpu().numpy() if isinstance(gain, torch.Tensor) else gain
        y = apply_gain_host(wav.detach().float().numpy() if tensor else wav, g, lengths, channels)
        return torch.from_numpy(y).to(wav.dtype) if tensor else y
    xf, lead, N, C, T = _meter_rows(wav, channels, 'apply_gain')
    gain = torch.as_tensor(gain, dtype=torch.float32, device=wav.device).reshape(-1).contiguous()
    if gain.numel() != N:
        raise _lib.PsndError('apply_gain: %d gains for %d programmes' % (gain.numel(), N))
    lengths = _device_lengths(lengths, N, wav.device, 'apply_gain')
    if out is None:
        y = torch.empty((N * C, T), dtype=torch.float32, device=wav.device)
    else:
        if out.dtype != torch.float32 or out.shape != wav.shape or not out.is_cuda or not out.is_contiguous():
            raise _lib.PsndError('apply_gain: out must be a contiguous float32 HIP tensor of the shape %s' % (tuple(wav.shape),))
        y = out
    if N * C * T > 0:
        with on(wav.device) as hip:
            hip.psnd_gain_rows(xf, N, C, T, lengths, gain, y)
    return out if out is not None else y.reshape(wav.shape).to(wav.dtype)


# ---- separation metrics (include/psnd.h: SNR / SI-SDR / SD-SDR, permutation-invariant matching, mixing at an SNR) ---------------------------
SEP_KINDS = ('snr', 'si_sdr', 'sd_sdr')                  # the `kind` of the C ABI is the index
SEP_EPS = float(np.finfo(np.float32).eps)                # torchmetrics' choice


def sep_span():
    """psnd_sep_span: the samples of a row per workgroup of the moment launch, the one size the kernel's seams depend on"""
    return int(lib().psnd_sep_span())


def sep_max_sources():
    """psnd_sep_max_sources: the most sources per item the permutation search takes"""
    return int(lib().psnd_sep_max_sources())


def _sep_config(kind, zero_mean, eps, who='sep_metric'):
    if kind not in SEP_KINDS:
        raise ValueError("%s: kind=%r - 'snr', 'si_sdr' or 'sd_sdr'" % (who, kind))
    eps = SEP_EPS if eps is None else float(eps)
    if not (math.isfinite(eps) and eps >= 0.0):
        raise ValueError('%s: eps=%r - finite, at least 0' % (who, eps))
    return SEP_KINDS.index(kind), int(bool(zero_mean)), eps


def _sep_shape(est, target, who):
    """(leading shape, B, S, T) of estimates and targets (..., S, T)"""
    if tuple(est.shape) != tuple(target.shape) or len(est.shape) < 2:
        raise _lib.PsndError('%s: estimates and targets (..., S, T) of one shape expected, got %s and %s'
                             % (who, tuple(est.shape), tuple(target.shape)))
    lead = tuple(est.shape[:-2])
    S, T = int(est.shape[-2]), int(est.shape[-1])
    if S < 1:
        raise _lib.PsndError('%s: S=%d sources' % (who, S))
    return lead, math.prod(lead), S, T


def sep_pair_values(kind, ee, ss, es, eps):
    """the pair value of include/psnd.h in float64 numpy from the (centred) moments, any broadcastable shapes: dB in float64"""
    ee, ss, es = (np.asarray(v, dtype=np.float64) for v in (ee, ss, es))
    with np.errstate(divide='ignore', invalid='ignore'):
        if kind == 'snr':
            return 10.0 * np.log10((ss + eps) / (np.maximum(ss - 2.0 * es + ee, 0.0) + eps))
        a = (es + eps) / (ss + eps)
        tg = a * a * ss
        n = tg - 2.0 * a * es + ee if kind == 'si_sdr' else ss - 2.0 * es + ee
        return 10.0 * np.log10((tg + eps) / (np.maximum(n, 0.0) + eps))


def sep_best_perm(pv):
    """the permutation p that maximises sum_i pv[i][p[i]] of a float32 pair matrix (S, S) - the values added in float64 in ascending i, the
    permutations walked in lexicographic order, a later one winning only by a strictly larger sum - as a list"""
    import itertools
    S = pv.shape[0]
    best, top = list(range(S)), None
    for p in itertools.permutations(range(S)):
        s = 0.0
        for i in range(S):
            s += float(pv[i, p[i]])
        if top is None or s > top:
            best, top = list(p), s
    return best


def sep_metric_host(est, target, kind, zero_mean=False, eps=None, lengths=None, pit=False, return_perm=False, return_pairs=False):
    """the definition of include/psnd.h in float64 numpy on arrays (..., S, T): float32 values (..., S) in dB - estimate i against target
    perm[i] - and on request the int32 permutation (..., S) and the float32 pair matrix (..., S, S).  The moments are taken of the explicitly
    centred rows (zero_mean), so nothing is lost to a difference.  An item that holds a non-finite sample before its length reads NaN and the
    identity permutation."""
    _sep_config(kind, zero_mean, eps)
    eps = SEP_EPS if eps is None else float(eps)
    est, target = np.asarray(est), np.asarray(target)
    lead, B, S, T = _sep_shape(est, target, 'sep_metric')
    lens = _host_lengths(lengths, B, T, 'sep_metric')
    E, G = est.reshape(B, S, T), target.reshape(B, S, T)
    value = np.zeros((B, S), dtype=np.float32)
    perm = np.tile(np.arange(S, dtype=np.int32), (B, 1))
    pair = np.zeros((B, S, S), dtype=np.float32)
    for b in range(B):
        e, s = E[b, :, :lens[b]].astype(np.float64), G[b, :, :lens[b]].astype(np.float64)
        if not (np.isfinite(e).all() and np.isfinite(s).all()):
            value[b], pair[b] = np.nan, np.nan
            continue
        if zero_mean and lens[b] > 0:
            e, s = e - e.mean(axis=-1, keepdims=True), s - s.mean(axis=-1, keepdims=True)
        ee, ss, es = (e * e).sum(axis=-1), (s * s).sum(axis=-1), e @ s.T
        pair[b] = sep_pair_values(kind, ee[:, None], ss[None, :], es, eps).astype(np.float32)
        if pit:
            perm[b] = sep_best_perm(pair[b])
        value[b] = pair[b][np.arange(S), perm[b]]
    out = (value.reshape(lead + (S,)),) + ((perm.reshape(lead + (S,)),) if return_perm else ()) \
        + ((pair.reshape(lead + (S, S)),) if return_pairs else ())
    return out if len(out) > 1 else out[0]


def _sep_rows(x, B, S, T):
    """a HIP tensor (..., S, T) as (B, S, T) float32 rows the kernels can walk where they lie: any 4-byte start, unit stride in time, rows T apart"""
    xf = x.reshape(B, S, T)
    if xf.dtype != torch.float32:
        xf = xf.float()
    if B * S * T > 0 and (xf.stride(2) != 1 or (S > 1 and xf.stride(1) != T) or (B > 1 and xf.stride(0) != S * T)):
        xf = xf.contiguous()
    return xf


class _SepMetric(torch.autograd.Function):
    """psnd_sep_metric_fwd / _bwd on (B, S, T) float32 rows: (loss or None, value, perm, pair or None, nan_flag or None).  Keeps `stats` and
    `perm` for the backward; differentiable in the estimates and the targets through the loss and through the values."""

    @staticmethod
    def forward(ctx, est, target, lengths, kind, zero_mean, eps, pit, want_pair, want_loss):
        B, S, T = est.shape
        dev = est.device
        value = torch.empty((B, S), dtype=torch.float32, device=dev)
        perm = torch.empty((B, S), dtype=torch.int32, device=dev)
        pair = torch.empty((B, S, S), dtype=torch.float32, device=dev) if want_pair else None
        loss = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
        flag = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
        stats = torch.empty(int(lib().psnd_sep_stats_doubles(B, S)), dtype=torch.float64, device=dev)
        scratch = torch.empty(int(lib().psnd_sep_scratch_bytes(B, S, T)) // 8, dtype=torch.float64, device=dev)
        with on(dev) as hip:
            hip.psnd_sep_metric_fwd(est, target, B, S, T, lengths, kind, zero_mean, eps, int(bool(pit)), scratch, stats, value, perm, pair,
                                    loss, flag)
        ctx.save_for_backward(est, target, stats, perm)
        ctx.cfg = (kind, zero_mean, eps)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*[t for t in (perm, pair, flag) if t is not None])
        return loss, value, perm, pair, flag

    @staticmethod
    def backward(ctx, g_loss, g_value, *_):
        est, target, stats, perm = ctx.saved_tensors
        if g_loss is None and g_value is None:
            return (None,) * 9
        B, S, T = est.shape
        kind, zero_mean, eps = ctx.cfg
        g_loss = None if g_loss is None else g_loss.to(torch.float32).contiguous()
        g_value = None if g_value is None else g_value.to(torch.float32).contiguous()
        g_est = torch.empty((B, S, T), dtype=torch.float32, device=est.device)
        g_target = torch.empty((B, S, T), dtype=torch.float32, device=est.device) if ctx.needs_input_grad[1] else None
        with on(est.device) as hip:
            hip.psnd_sep_metric_bwd(est, target, B, S, T, kind, zero_mean, eps, stats, perm, g_loss, g_value, g_est, g_target)
        return (g_est if ctx.needs_input_grad[0] else None, g_target) + (None,) * 7


def sep_metric_loss(est, target, kind, zero_mean=False, eps=None, lengths=None, pit=False, return_pairs=False, want_loss=True):
    """one call of psnd_sep_metric_fwd on HIP tensors (..., S, T): (loss, value, perm, pair, nan_flag) - the scalar -mean(value) and
    isnan(loss) as float32 device scalars (None without want_loss), float32 values and int32 permutation (..., S), the pair matrix
    (..., S, S) or None.  Differentiable in both inputs through `loss` and `value`; nothing is read back by the host."""
    if not (isinstance(est, torch.Tensor) and isinstance(target, torch.Tensor) and est.is_cuda and target.is_cuda):
        raise _lib.PsndError('sep_metric: HIP tensors are expected here (CPU tensors and numpy arrays take sep_metric_host)')
    if not (est.is_floating_point() and target.is_floating_point()):
        raise _lib.PsndError('sep_metric: floating inputs expected, got %s and %s' % (est.dtype, target.dtype))
    k, zm, eps = _sep_config(kind, zero_mean, eps)
    lead, B, S, T = _sep_shape(est, target, 'sep_metric')
    if S > sep_max_sources():
        raise _lib.PsndError('sep_metric: S=%d sources, the permutation search takes at most %d' % (S, sep_max_sources()))
    lengths = _device_lengths(lengths, B, est.device, 'sep_metric')
    if B * T == 0:                                       # nothing to launch: the formulas on zero moments; no sample, no gradient
        host = sep_metric_host(np.zeros((B, S, T), np.float32), np.zeros((B, S, T), np.float32), kind, zero_mean, eps, None, pit, True, True)
        value, perm, pair = (torch.from_numpy(v).to(est.device) for v in host)
        loss = -value.mean() if B else torch.zeros((), device=est.device)
        flag = torch.isnan(loss).float()
    else:
        e, t = _sep_rows(est, B, S, T), _sep_rows(target, B, S, T)
        loss, value, perm, pair, flag = _SepMetric.apply(e, t, lengths, k, zm, eps, bool(pit), bool(return_pairs), bool(want_loss))
    pair = pair.reshape(lead + (S, S)) if return_pairs else None
    return (loss, value.reshape(lead + (S,)), perm.reshape(lead + (S,)), pair, flag) if want_loss else \
        (None, value.reshape(lead + (S,)), perm.reshape(lead + (S,)), pair, None)


def sep_metric(est, target, kind, zero_mean=False, eps=None, lengths=None, pit=False, return_perm=False, return_pairs=False):
    """SNR ('snr'), scale-invariant SDR ('si_sdr') or scale-dependent SDR ('sd_sdr') in dB of S estimates against S targets per item, the
    definition of include/psnd.h: `est`, `target` (..., S, T) -> float32 values (..., S).  `zero_mean`: take the means out first; `eps`: the
    regulariser (default float32 machine epsilon); `lengths`: per-ITEM valid lengths (leading shape), clamped to [0, T]; `pit`: match the
    estimates with the targets by the permutation that maximises the sum of the values (estimate i with target perm[i], ties to the
    lexicographically first).  return_perm / return_pairs: also the int32 permutation (..., S) / the whole float32 pair matrix
    (..., S, S), in that order.  An item that holds a non-finite sample reads NaN and the identity permutation.

    HIP tensors run psnd_separation.hip - at most three launches forward (without the loss: two), one backward, no host synchronisation -
    and carry a gradient to the estimates and the targets; numpy arrays and CPU tensors go through `sep_metric_host` in float64, without
    a gradient."""
    if isinstance(est, torch.Tensor) and est.is_cuda:
        _, value, perm, pair, _ = sep_metric_loss(est, target, kind, zero_mean, eps, lengths, pit, return_pairs, want_loss=False)
        out = (value,) + ((perm,) if return_perm else ()) + ((pair,) if return_pairs else ())
        return out if len(out) > 1 else out[0]
    tensor = isinstance(est, torch.Tensor)
    to_np = lambda v: v.detach().to(torch.float64 if v.dtype == torch.bfloat16 else v.dtype).cpu().numpy() if isinstance(v, torch.Tensor) else v  # noqa: E731
    r = sep_metric_host(to_np(est), to_np(target), kind, zero_mean, eps, lengths, pit, return_perm, return_pairs)
    if not tensor:
        return r
    return tuple(torch.from_numpy(np.array(v)) for v in r) if isinstance(r, tuple) else torch.from_numpy(np.array(r))


def mix_at_snr_host(x, z, snr, lengths=None):
    """torchaudio's add_noise by the definition of include/psnd.h in numpy: x + g z before a row's length with g = sqrt(sum x^2 / sum z^2)
    10^(-snr / 20) in float64, rounded to float32, x behind it; g = 0 for a silent or non-finite row.  (float32 result, the float32 gains)"""
    x, z = np.asarray(x), np.asarray(z)
    if x.shape != z.shape or x.ndim < 1:
        raise _lib.PsndError('mix_at_snr: signal and noise (..., T) of one shape expected, got %s and %s' % (x.shape, z.shape))
    T = int(x.shape[-1])
    R = math.prod(x.shape[:-1])
    lens = _host_lengths(lengths, R, T, 'mix_at_snr')
    snr = np.asarray(snr, dtype=np.float32).reshape(-1)
    if snr.size not in (1, R):
        raise _lib.PsndError('mix_at_snr: %d SNRs for %d rows' % (snr.size, R))
    xf, zf = x.reshape(R, T).astype(np.float32), z.reshape(R, T).astype(np.float32)
    y, gain = xf.copy(), np.zeros(R, dtype=np.float32)
    for r in range(R):
        a, b = xf[r, :lens[r]].astype(np.float64), zf[r, :lens[r]].astype(np.float64)
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            continue
        xx, zz = float((a * a).sum()), float((b * b).sum())
        if xx > 0.0 and zz > 0.0:
            with np.errstate(over='ignore'):
                gain[r] = np.float32(math.sqrt(xx / zz) * np.power(10.0, -np.float64(snr[r if snr.size > 1 else 0]) / 20.0))
            y[r, :lens[r]] = (a + np.float64(gain[r]) * b).astype(np.float32)
    return y.reshape(x.shape), gain.reshape(x.shape[:-1])


def mix_at_snr(x, z, snr, lengths=None, out=None, return_gain=False):
    """`x` with the noise `z` added at `snr` dB (torchaudio's add_noise, include/psnd.h): x + g z before a row's length, x behind it, with
    g = sqrt(sum x^2 / sum z^2) 10^(-snr / 20) per row of (..., T); `snr`: one number or one per row (a tensor stays on its device).  A row
    that is silent in either input or holds a non-finite sample comes back unchanged (g = 0).  On HIP tensors psnd_snr_gain and
    psnd_mix_rows: three launches, the gain never leaves the device, capturable; `out`: a contiguous float32 HIP tensor of x's shape, `x`
    itself for in place.  numpy arrays and CPU tensors go through `mix_at_snr_host`.  No gradient."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda):
        if out is not None:
            raise _lib.PsndError('mix_at_snr: out= is for HIP tensors')
        tensor = isinstance(x, torch.Tensor)
        to_np = lambda v: v.detach().float().cpu().numpy() if isinstance(v, torch.Tensor) else v  # noqa: E731
        y, g = mix_at_snr_host(to_np(x), to_np(z), to_np(snr), lengths)
        if tensor:
            y, g = torch.from_numpy(y).to(x.dtype), torch.from_numpy(np.array(g))
        return (y, g) if return_gain else y
    if not (isinstance(z, torch.Tensor) and z.is_cuda) or x.shape != z.shape:
        raise _lib.PsndError('mix_at_snr: signal and noise of one shape on one device expected')
    xf, lead, R, _, T = _meter_rows(x, None, 'mix_at_snr')
    zf = _meter_rows(z, None, 'mix_at_snr')[0]
    dev = x.device
    snr = torch.as_tensor(snr, dtype=torch.float32).reshape(-1)
    if snr.numel() not in (1, R):
        raise _lib.PsndError('mix_at_snr: %d SNRs for %d rows' % (snr.numel(), R))
    snr = snr.to(dev).contiguous()
    lengths = _device_lengths(lengths, R, dev, 'mix_at_snr')
    if out is None:
        y = torch.empty((R, T), dtype=torch.float32, device=dev)
    else:
        if out.dtype != torch.float32 or out.shape != x.shape or not out.is_cuda or not out.is_contiguous():
            raise _lib.PsndError('mix_at_snr: out must be a contiguous float32 HIP tensor of the shape %s' % (tuple(x.shape),))
        y = out
    gain = torch.zeros(R, dtype=torch.float32, device=dev)
    if R * T > 0:
        scratch = torch.empty(int(lib().psnd_sep_scratch_bytes(R, 1, T)) // 8, dtype=torch.float64, device=dev)
        with on(dev) as hip:
            hip.psnd_snr_gain(xf, zf, R, T, lengths, snr, snr.numel(), scratch, gain)
            hip.psnd_mix_rows(xf, zf, R, T, lengths, gain, y)
    y = out if out is not None else y.reshape(x.shape).to(x.dtype)
    return (y, gain.reshape(lead)) if return_gain else y


def _count(name, v, least):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < least:
        raise ValueError('yin: %s=%r - a count of samples, at least %d' % (name, v, least))
    return int(v)


def yin_lags(sr, f0_floor=71.0, f0_ceil=800.0, frame_length=None):
    """(tau_min, tau_max, W) of include/psnd.h from a search range in Hz: tau_min = max(2, floor(sr / f0_ceil)), tau_max = ceil(sr / f0_floor),
    W = frame_length or 2 tau_max.  ValueError on a rate or a range that is not positive and finite, an empty range, or W < tau_max."""
    sr, lo, hi = float(sr), float(f0_floor), float(f0_ceil)
    for name, v in (('sr', sr), ('f0_floor', lo), ('f0_ceil', hi)):
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError('yin: %s=%r - positive and finite' % (name, v))
    if sr / lo > 2.0 ** 31:
        raise ValueError('yin: f0_floor=%r at sr=%r is a lag of more than 2^31 samples' % (lo, sr))
    tau_min, tau_max = max(2, math.floor(sr / hi)), math.ceil(sr / lo)
    if tau_max < tau_min:
        raise ValueError('yin: no lag between f0_ceil=%r and f0_floor=%r at sr=%r (tau_min=%d, tau_max=%d)' % (hi, lo, sr, tau_min, tau_max))
    W = 2 * tau_max if frame_length is None else _count('frame_length', frame_length, 1)
    if W < tau_max:
        raise ValueError('yin: frame_length=%d is shorter than the longest lag tau_max=%d' % (W, tau_max))
    return tau_min, tau_max, W


def yin_frames(T, hop):
    """psnd_yin_frames: T // hop + 1 frames, at the samples 0, hop, 2 hop, ..."""
    return int(T) // _count('hop', hop, 1) + 1


def yin_threshold(threshold):
    th = float(threshold)
    if not th > 0.0:
        raise ValueError('yin: threshold=%r - positive' % (threshold,))
    return th


def yin_f0_host(x, hop, sr, tau_min, tau_max, W, threshold, chunk=256):
    """the definition of include/psnd.h (YIN steps 1-5 and the non-finite rule) on one row of numpy samples in float64, vectorised over the
    frames and over j, `chunk` frames at a time: (f0, aperiodicity, lag) as float64, float64, int32 arrays of yin_frames(T, hop) entries"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    T, F = x.shape[0], x.shape[0] // hop + 1
    span = W + tau_max
    H = span // 2
    xp = np.concatenate((np.zeros(H), x, np.zeros(span)))              # frame i reads xp[i hop : i hop + span]: i hop <= T
    f0, ap, lag = np.zeros(F), np.ones(F), np.zeros(F, dtype=np.int32)
    taus = np.arange(1, tau_max + 1)
    rng = (taus >= tau_min)
    for a in range(0, F, chunk):
        idx = np.arange(a, min(a + chunk, F))
        U = xp[idx[:, None] * hop + np.arange(span)]
        bad = ~np.isfinite(U).all(axis=1)
        U[bad] = 0.0
        d = np.empty((idx.size, tau_max))
        for tau in taus:
            e = U[:, :W] - U[:, tau:tau + W]
            d[:, tau - 1] = (e * e).sum(axis=1)
        cs = np.cumsum(d, axis=1)
        dp = np.where(cs == 0.0, 1.0, d * taus / np.where(cs == 0.0, 1.0, cs))
        under = (dp < threshold) & rng
        voiced = under.any(axis=1) & ~bad
        t0 = under.argmax(axis=1)                                       # index of the lag t0 = index + 1
        last = np.ones((idx.size, 1), dtype=bool)
        stop = np.concatenate((~(dp[:, 1:] < dp[:, :-1]), last), axis=1) & (np.arange(tau_max) >= t0[:, None])
        k = stop.argmax(axis=1)                                         # the descent ends at the lag k + 1
        rows = np.arange(idx.size)
        y1 = dp[rows, k]
        inner = (k >= 1) & (k + 1 <= tau_max - 1)
        y0, y2 = dp[rows, np.maximum(k - 1, 0)], dp[rows, np.minimum(k + 1, tau_max - 1)]
        den = y0 - 2.0 * y1 + y2
        ok = inner & (den > 0.0)
        off = np.where(ok, np.clip(0.5 * (y0 - y2) / np.where(ok, den, 1.0), -0.5, 0.5), 0.0)
        f0[idx] = np.where(voiced, sr / (k + 1 + off), 0.0)
        lag[idx] = np.where(voiced, k + 1, 0)
        ap[idx] = np.where(bad, 1.0, np.where(voiced, y1, np.where(rng, dp, np.inf).min(axis=1)))
    return f0, ap, lag


def yin_f0(wav, hop, sr=22050, f0_floor=71.0, f0_ceil=800.0, threshold=0.1, frame_length=None, lengths=None):
    """fundamental frequency per frame of every row of `wav` (..., T) by the definition of include/psnd.h (YIN, steps 1-5):
    (f0 float32, aperiodicity float32, lag int32), each (..., F) on wav's device, F = T // hop + 1, frame i at the sample i hop.  An
    unvoiced frame has f0 = 0 and lag = 0.  `lengths`: per-row valid lengths, clamped to [0, T]; row n then has lengths[n] // hop + 1 frames,
    its samples from lengths[n] on count as zeros and its remaining slots hold (0, 1, 0).

    HIP tensors run psnd_yin_f0 (float32; float16 / bfloat16 are cast; float64 raises) in one launch with no host synchronisation - the
    call can be captured; `lengths` is then an int64 tensor on the same device (anything else is copied there).  CPU tensors go through
    yin_f0_host in float64.  No autograd: a lag is an integer and f0 jumps with it."""
    if not isinstance(wav, torch.Tensor):
        raise _lib.PsndError('yin: a tensor is expected, got %s' % type(wav).__name__)
    if wav.dim() == 0:
        raise _lib.PsndError('yin: the input needs a time axis')
    if not wav.is_floating_point():
        raise _lib.PsndError('yin: floating input expected, got %s' % wav.dtype)
    hop = _count('hop', hop, 1)
    tau_min, tau_max, W = yin_lags(sr, f0_floor, f0_ceil, frame_length)
    th = yin_threshold(threshold)
    lead, T = tuple(wav.shape[:-1]), wav.shape[-1]
    N = math.prod(lead)
    F = yin_frames(T, hop)
    if lengths is not None:
        lengths = torch.as_tensor(lengths)
        if lengths.is_floating_point() or lengths.numel() != N:
            raise _lib.PsndError('yin: lengths must be %d integers, got %s %s' % (N, tuple(lengths.shape), lengths.dtype))
    if not wav.is_cuda:
        rows = wav.detach().reshape(N, T).to(torch.float64).numpy()
        lens = [T] * N if lengths is None else [min(max(int(v), 0), T) for v in lengths.reshape(-1).tolist()]
        f0, ap, lag = np.zeros((N, F), np.float32), np.ones((N, F), np.float32), np.zeros((N, F), np.int32)
        for n in range(N):
            r = yin_f0_host(rows[n, :lens[n]], hop, float(sr), tau_min, tau_max, W, th)
            f0[n, :r[0].size], ap[n, :r[0].size], lag[n, :r[0].size] = r
        return tuple(torch.from_numpy(a).reshape(lead + (F,)) for a in (f0, ap, lag))
    if wav.dtype == torch.float64:
        raise _lib.PsndError('yin: no float64 instance on HIP tensors (a round trip through float32 would silently change which lag passes '
                             'the threshold): pass a float32 tensor, or a CPU tensor in float64')
    if wav.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.PsndError('yin: floating input expected, got %s' % wav.dtype)
    xf = wav.detach().reshape(N, T).float()
    if N * T > 0 and (xf.stride(-1) != 1 or (N > 1 and xf.stride(0) != T)):
        xf = xf.contiguous()
    if lengths is not None:
        lengths = lengths.reshape(-1).to(device=wav.device, dtype=torch.int64).contiguous()
    f0 = torch.empty((N, F), dtype=torch.float32, device=wav.device)
    ap = torch.empty((N, F), dtype=torch.float32, device=wav.device)
    lag = torch.empty((N, F), dtype=torch.int32, device=wav.device)
    if N > 0:
        with on(wav.device) as hip:
            hip.psnd_yin_f0(xf if T > 0 else None, N, T, lengths, hop, W, tau_min, tau_max, th, float(sr), f0, ap, lag, F)
    return f0.reshape(lead + (F,)), ap.reshape(lead + (F,)), lag.reshape(lead + (F,))


def pv_pass():
    """psnd_pv_pass: the output frames a wave of psnd_phase_vocoder.hip takes per pass - the size its seams depend on"""
    return int(lib().psnd_pv_pass())


def _pv_rate(rate):
    try:
        r = float(rate)
    except (TypeError, ValueError):
        raise ValueError('phase_vocoder: rate=%r - a positive, finite number' % (rate,))
    if isinstance(rate, bool) or not (r > 0.0 and math.isfinite(r)):
        raise ValueError('phase_vocoder: rate=%r - a positive, finite number' % (rate,))
    return r


def pv_frames(F, rate):
    """psnd_pv_frames: the number of output frames j >= 0 with float(j) * rate < F, counted by that wording (a bare ceil(F / rate) is off
    by one where the product rounds)"""
    F, rate = int(F), _pv_rate(rate)
    if F <= 0:
        return 0
    q = math.ceil(F / rate)
    if q >= 2 ** 53:
        raise ValueError('phase_vocoder: F=%d at rate=%r is more than 2^53 output frames' % (F, rate))
    j = int(q)
    while j > 0 and not float(j - 1) * rate < F:
        j -= 1
    while float(j) * rate < F:
        j += 1
    return j


def pitch_ratio(n_steps, bins_per_octave=12):
    """(p, q): the fraction p / q closest in cents to 2 ** (n_steps / bins_per_octave) with max(p, q) <= 640 - the largest factor whose
    default resampling filter (20 max + 1 taps) fits RESAMPLE_MAX_TAPS -, ties to the smaller p.  utils.sound.pitch_shift shifts by THIS
    interval, not the irrational one; every semitone count up to an octave is met within 0.03 cent."""
    n, b = float(n_steps), float(bins_per_octave)
    if not math.isfinite(n) or not (b > 0.0 and math.isfinite(b)) or isinstance(bins_per_octave, bool):
        raise ValueError('pitch_ratio: n_steps=%r bins_per_octave=%r - a finite count of steps, a positive count per octave' % (n_steps, bins_per_octave))
    octaves = n / b
    top = (RESAMPLE_MAX_TAPS - 1) // 20
    if abs(octaves) > math.log2(top):
        raise ValueError('pitch_ratio: %r steps of %r per octave is beyond a factor of %d' % (n_steps, bins_per_octave, top))
    target = 2.0 ** octaves
    best, best_err = (1, 1), abs(octaves)
    for p in range(1, top + 1):
        q0 = p / target
        for q in (math.floor(q0), math.floor(q0) + 1):
            if 1 <= q <= top:
                err = abs(math.log2(p / q) - octaves)
                if err < best_err:
                    best, best_err = (p, q), err
    g = math.gcd(*best)
    return best[0] // g, best[1] // g


def phase_vocoder_host(re, im, rate, frames=None):
    """the definition of include/psnd.h on float64 numpy arrays (..., F), vectorised over the rows and the output frames: (yre, yim), each
    (..., pv_frames(F, rate)).  `frames`: valid input frames per row of the arrays flattened to (rows, F) - one entry per row, or anything
    that broadcasts against the leading axes -, clamped to [0, F]."""
    rate = _pv_rate(rate)
    re, im = np.asarray(re, dtype=np.float64), np.asarray(im, dtype=np.float64)
    if re.shape != im.shape or re.ndim == 0:
        raise ValueError('phase_vocoder: re %s and im %s must have one shape with a frame axis' % (re.shape, im.shape))
    lead, F = re.shape[:-1], re.shape[-1]
    J = pv_frames(F, rate)
    Fn = np.full(lead, F, dtype=np.int64) if frames is None else np.clip(np.broadcast_to(np.asarray(frames, dtype=np.int64), lead), 0, F)
    live = np.arange(F + 1) < Fn[..., None]                                  # one frame of zeros behind the row
    xr = np.where(live, np.concatenate((re, np.zeros(lead + (1,))), axis=-1), 0.0)
    xi = np.where(live, np.concatenate((im, np.zeros(lead + (1,))), axis=-1), 0.0)
    t = np.arange(J, dtype=np.float64) * rate
    i = np.floor(t).astype(np.int64)
    alpha = t - i
    with np.errstate(invalid='ignore', over='ignore'):
        mag = np.hypot(xr, xi)
        ang = np.where((xr == 0.0) & (xi == 0.0), 0.0, np.arctan2(xi, xr))
        lost = ~(np.isfinite(xr) & np.isfinite(xi))
        step = ang[..., i + 1] - ang[..., i]
        phi = ang[..., :1] + np.concatenate((np.zeros(lead + (min(J, 1),)), np.cumsum(step[..., :-1], axis=-1)), axis=-1)
        m = (1.0 - alpha) * mag[..., i] + alpha * mag[..., i + 1]
        yre, yim = m * np.cos(phi), m * np.sin(phi)
    nan = np.logical_or.accumulate(lost[..., i] | lost[..., i + 1], axis=-1)
    valid = t < Fn[..., None]
    yre = np.where(valid, np.where(nan, np.nan, yre), 0.0)
    yim = np.where(valid, np.where(nan, np.nan, yim), 0.0)
    return yre, yim


def phase_vocoder(re, im, rate, frames=None):
    """time-scale modification of the spectrogram re + i im, tensors (..., K, F) as STFT.transform_complex returns them, by the definition
    of include/psnd.h: output frame j stands at the input time j rate, its magnitude interpolated between the frames floor(j rate) and
    floor(j rate) + 1, its phase advanced by the angle between the two frames the frame before it read.  Returns (yre, yim), each
    (..., K, pv_frames(F, rate)) in the inputs' dtype and on their device.  rate > 1 shortens, rate < 1 lengthens.  `frames`: valid input
    frames per batch item (one integer per leading index, clamped to [0, F]); an item's frames from there on count as zeros and its output
    slots from pv_frames(frames[n], rate) on hold zeros.  A row that reads a NaN or an Inf is NaN from that output frame on.

    HIP tensors run psnd_phase_vocoder (float32; float16 / bfloat16 are cast in and out; float64 raises) in one launch with no host
    synchronisation - the call can be captured; `frames` is then an int64 tensor on the same device (anything else is copied there).  CPU
    tensors go through phase_vocoder_host in float64.  No autograd: the outputs carry no graph, gradients are out of scope."""
    if not isinstance(re, torch.Tensor) or not isinstance(im, torch.Tensor):
        raise _lib.PsndError('phase_vocoder: tensors are expected, got %s and %s' % (type(re).__name__, type(im).__name__))
    if re.shape != im.shape or re.dtype != im.dtype or re.device != im.device:
        raise _lib.PsndError('phase_vocoder: re (%s %s %s) and im (%s %s %s) must agree' % (tuple(re.shape), re.dtype, re.device, tuple(im.shape),
                                                                                          im.dtype, im.device))
    if re.dim() < 2:
        raise _lib.PsndError('phase_vocoder: (..., K, F) expected, got %s' % (tuple(re.shape),))
    if not re.is_floating_point():
        raise _lib.PsndError('phase_vocoder: floating input expected, got %s' % re.dtype)
    rate = _pv_rate(rate)
    lead, K, F = tuple(re.shape[:-2]), re.shape[-2], re.shape[-1]
    N = math.prod(lead)
    J = pv_frames(F, rate)
    if J >= 2 ** 31:
        raise _lib.PsndError('phase_vocoder: F=%d at rate=%r is %d output frames, 2^31 or more' % (F, rate, J))
    if frames is not None:
        frames = torch.as_tensor(frames)
        if frames.is_floating_point() or frames.numel() != N:
            raise _lib.PsndError('phase_vocoder: frames must be %d integers, got %s %s' % (N, tuple(frames.shape), frames.dtype))
    out_shape = lead + (K, J)
    if not re.is_cuda:
        fr = None if frames is None else frames.reshape(N, 1).numpy()
        yr, yi = phase_vocoder_host(re.detach().reshape(N, K, F).to(torch.float64).numpy(), im.detach().reshape(N, K, F).to(torch.float64).numpy(),
                                    rate, fr)
        return tuple(torch.from_numpy(np.ascontiguousarray(y)).to(re.dtype).reshape(out_shape) for y in (yr, yi))
    if re.dtype == torch.float64:
        raise _lib.PsndError('phase_vocoder: no float64 instance on HIP tensors (a round trip through float32 would silently lose the '
                             'precision asked for): pass float32 tensors, or CPU tensors in float64')
    if re.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.PsndError('phase_vocoder: floating input expected, got %s' % re.dtype)
    xr, xi = (t.detach().reshape(N, K, F).float().contiguous() for t in (re, im))
    if frames is not None:
        frames = frames.reshape(-1).to(device=re.device, dtype=torch.int64).contiguous()
    yr = torch.empty((N, K, J), dtype=torch.float32, device=re.device)
    yi = torch.empty((N, K, J), dtype=torch.float32, device=re.device)
    if N * K * J > 0:
        with on(re.device) as hip:
            hip.psnd_phase_vocoder(xr if F > 0 else None, xi if F > 0 else None, N, K, F, frames, rate, yr, yi, J)
    return yr.to(re.dtype).reshape(out_shape), yi.to(re.dtype).reshape(out_shape)


GL_EPS = 1e-16


def gl_chunk():
    """psnd_gl_chunk: the elements of an item a workgroup of psnd_griffinlim.hip takes - the size its seams depend on"""
    return int(lib().psnd_gl_chunk())


def gl_chunks(K, F):
    """psnd_gl_chunks: the chunks per item, ceil(K F / gl_chunk()) - the middle axis of the step's `partial`"""
    return int(lib().psnd_gl_chunks(int(K), int(F)))


def _gl_host_frames(frames, N, F):
    if frames is None:
        return np.full((N,), F, dtype=np.int64)
    return np.clip(np.asarray(frames, dtype=np.int64).reshape(N), 0, F)


def griffinlim_start_host(mag, phase=None, frames=None):
    """the start of include/psnd.h's Griffin-Lim section on float64 numpy arrays (N, K, F): X0 = S (cos phi, sin phi), (S, 0) without a
    phase, (0, 0) at f >= frames[n]"""
    S = np.asarray(mag, dtype=np.float64)
    if S.ndim != 3:
        raise ValueError('griffinlim_start: (N, K, F) expected, got %s' % (S.shape,))
    N, _, F = S.shape
    live = np.arange(F)[None, None, :] < _gl_host_frames(frames, N, F)[:, None, None]
    if phase is None:
        return np.where(live, S, 0.0), np.zeros_like(S)
    phi = np.asarray(phase, dtype=np.float64)
    if phi.shape != S.shape:
        raise ValueError('griffinlim_start: mag %s and phase %s must have one shape' % (S.shape, phi.shape))
    with np.errstate(invalid='ignore', over='ignore'):
        return np.where(live, S * np.cos(phi), 0.0), np.where(live, S * np.sin(phi), 0.0)


def griffinlim_step_host(mag, cre, cim, pre=None, pim=None, alpha=0.0, eps=GL_EPS, frames=None):
    """the step of include/psnd.h's Griffin-Lim section on float64 numpy arrays (N, K, F): t = C - alpha P (t = C without P),
    X = S (t / (hypot(t) + eps)), (0, 0) at f >= frames[n].  Returns (xre, xim, sums) with sums (N, 2) = the sums of (|C| - S)^2 and of S^2
    over the valid elements of each item."""
    S, cr, ci = (np.asarray(a, dtype=np.float64) for a in (mag, cre, cim))
    if S.ndim != 3 or cr.shape != S.shape or ci.shape != S.shape:
        raise ValueError('griffinlim_step: mag, cre, cim must share one (N, K, F) shape, got %s %s %s' % (S.shape, cr.shape, ci.shape))
    if (pre is None) != (pim is None):
        raise ValueError('griffinlim_step: pre and pim come together or not at all')
    N, _, F = S.shape
    live = np.arange(F)[None, None, :] < _gl_host_frames(frames, N, F)[:, None, None]
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        tr, ti = cr, ci
        if pre is not None:
            pr, pi = np.asarray(pre, dtype=np.float64), np.asarray(pim, dtype=np.float64)
            if pr.shape != S.shape or pi.shape != S.shape:
                raise ValueError('griffinlim_step: pre %s and pim %s must have the shape of mag %s' % (pr.shape, pi.shape, S.shape))
            tr, ti = cr - alpha * pr, ci - alpha * pi
        den = np.hypot(tr, ti) + eps
        xr = np.where(live, S * (tr / den), 0.0)
        xi = np.where(live, S * (ti / den), 0.0)
        d = np.where(live, np.hypot(cr, ci) - S, 0.0)
        q = np.where(live, S, 0.0)
        sums = np.stack(((d * d).sum(axis=(1, 2)), (q * q).sum(axis=(1, 2))), axis=-1)
    return xr, xi, sums


def _gl_planes(who, named, frames):
    """shape, dtype and device checks shared by griffinlim_start / griffinlim_step: `named` = [(name, tensor or None)], the first one is
    the magnitude.  Returns (lead, N, K, F, frames as they go to the entry point)"""
    first = named[0][1]
    for name, t in named:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise _lib.PsndError('%s: tensors are expected, %s is a %s' % (who, name, type(t).__name__))
        if t.shape != first.shape or t.dtype != first.dtype or t.device != first.device:
            raise _lib.PsndError('%s: %s (%s %s %s) must agree with %s (%s %s %s)' % (who, name, tuple(t.shape), t.dtype, t.device, named[0][0],
                                                                                    tuple(first.shape), first.dtype, first.device))
    if first.dim() < 2:
        raise _lib.PsndError('%s: (..., K, F) expected, got %s' % (who, tuple(first.shape)))
    if not first.is_floating_point():
        raise _lib.PsndError('%s: floating input expected, got %s' % (who, first.dtype))
    if first.is_cuda and first.dtype == torch.float64:
        raise _lib.PsndError('%s: no float64 instance on HIP tensors (a round trip through float32 would silently lose the precision asked '
                             'for): pass float32 tensors, or CPU tensors in float64' % who)
    if first.is_cuda and first.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.PsndError('%s: floating input expected, got %s' % (who, first.dtype))
    lead, K, F = tuple(first.shape[:-2]), first.shape[-2], first.shape[-1]
    N = math.prod(lead)
    if frames is not None:
        frames = torch.as_tensor(frames)
        if frames.is_floating_point() or frames.dtype == torch.bool or frames.numel() != N:
            raise _lib.PsndError('%s: frames must be %d integers, got %s %s' % (who, N, tuple(frames.shape), frames.dtype))
        frames = frames.reshape(-1).to(device=first.device, dtype=torch.int64).contiguous()
    return lead, N, K, F, frames


def _gl_out(who, out, N, K, F, device):
    if out is None:
        return (torch.empty((N, K, F), dtype=torch.float32, device=device), torch.empty((N, K, F), dtype=torch.float32, device=device))
    for t in out:
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and t.numel() == N * K * F and t.is_contiguous()):
            raise _lib.PsndError('%s: out must be two contiguous float32 tensors of %d elements on %s' % (who, N * K * F, device))
    return out


def griffinlim_start(mag, phase=None, frames=None):
    """X0 of Griffin-Lim (include/psnd.h): (xre, xim) = mag (cos phase, sin phase), or (mag, 0) without a phase, tensors (..., K, F) in
    mag's dtype and on its device; `frames`: valid frames per batch item (one integer per leading index, clamped to [0, F]) - an item's
    elements from there on are never read and come out as (0, 0).  HIP tensors run psnd_griffinlim_start (float32; float16 / bfloat16 are cast
    in and out; float64 raises) in one launch; CPU tensors go through griffinlim_start_host in float64.  No autograd."""
    lead, N, K, F, frames = _gl_planes('griffinlim_start', [('mag', mag), ('phase', phase)], frames)
    if not mag.is_cuda:
        fr = None if frames is None else frames.numpy()
        xr, xi = griffinlim_start_host(mag.detach().reshape(N, K, F).to(torch.float64).numpy(),
                                       None if phase is None else phase.detach().reshape(N, K, F).to(torch.float64).numpy(), fr)
        return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(mag.dtype).reshape(mag.shape) for x in (xr, xi))
    S = mag.detach().reshape(N, K, F).float().contiguous()
    phi = None if phase is None else phase.detach().reshape(N, K, F).float().contiguous()
    xr, xi = _gl_out('griffinlim_start', None, N, K, F, mag.device)
    if N * K * F > 0:
        with on(mag.device) as hip:
            hip.psnd_griffinlim_start(S, phi, N, K, F, frames, xr, xi)
    return xr.to(mag.dtype).reshape(mag.shape), xi.to(mag.dtype).reshape(mag.shape)


def griffinlim_step(mag, cre, cim, pre=None, pim=None, alpha=0.0, eps=GL_EPS, frames=None, out=None, partial=False):
    """one phase step of Griffin-Lim (include/psnd.h): with t = (cre, cim) - alpha (pre, pim) - or t = (cre, cim) without pre / pim -
    (xre, xim) = mag (t / (hypot(t) + eps)), tensors (..., K, F) in mag's dtype and on its device.  `frames` as in griffinlim_start.
    `partial=True` also returns the sums of (|C| - mag)^2 and mag^2 over the valid elements: on HIP tensors the kernel's own
    (N, gl_chunks(K, F), 2) float32 tensor of per-chunk sums (a float32 tensor of that shape may be passed instead and is written), on CPU
    tensors one float64 pair per item, (N, 1, 2).

    HIP tensors run psnd_griffinlim_step (float32; float16 / bfloat16 are cast in and out; float64 raises; non-contiguous input is made
    contiguous) in one launch with no host synchronisation - the call can be captured.  `out`: two contiguous float32 tensors of the input's
    size to write into (float32 input only); they may be the very tensors pre / pim, nothing else of the input.  CPU tensors go through
    griffinlim_step_host in float64.  No autograd."""
    who = 'griffinlim_step'
    if (pre is None) != (pim is None):
        raise _lib.PsndError('%s: pre and pim come together or not at all' % who)
    lead, N, K, F, frames = _gl_planes(who, [('mag', mag), ('cre', cre), ('cim', cim), ('pre', pre), ('pim', pim)], frames)
    alpha, eps = float(alpha), float(eps)
    if not mag.is_cuda:
        if out is not None:
            raise _lib.PsndError('%s: out is for HIP tensors' % who)
        f64 = lambda t: None if t is None else t.detach().reshape(N, K, F).to(torch.float64).numpy()       # noqa: E731
        xr, xi, sums = griffinlim_step_host(f64(mag), f64(cre), f64(cim), f64(pre), f64(pim), alpha, eps, None if frames is None else frames.numpy())
        res = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(mag.dtype).reshape(mag.shape) for x in (xr, xi))
        return res + (torch.from_numpy(sums).reshape(N, 1, 2),) if partial is not False and partial is not None else res
    if out is not None and mag.dtype != torch.float32:
        raise _lib.PsndError('%s: out goes with float32 input, got %s' % (who, mag.dtype))
    f32 = lambda t: None if t is None else t.detach().reshape(N, K, F).float().contiguous()                  # noqa: E731
    S, cr, ci, pr, pi = f32(mag), f32(cre), f32(cim), f32(pre), f32(pim)
    xr, xi = _gl_out(who, out, N, K, F, mag.device)
    part = None
    if isinstance(partial, torch.Tensor):
        part = partial
        if part.dtype != torch.float32 or part.device != mag.device or not part.is_contiguous() or tuple(part.shape) != (N, gl_chunks(K, F), 2):
            raise _lib.PsndError('%s: partial must be a contiguous float32 (%d, %d, 2) tensor on %s' % (who, N, gl_chunks(K, F), mag.device))
    elif partial:
        part = torch.empty((N, gl_chunks(K, F), 2), dtype=torch.float32, device=mag.device)
    if N * K * F > 0:
        with on(mag.device) as hip:
            hip.psnd_griffinlim_step(S, cr, ci, pr, pi, N, K, F, frames, alpha, eps, xr, xi, part)
    res = (xr.reshape(mag.shape), xi.reshape(mag.shape)) if out is not None else (xr.to(mag.dtype).reshape(mag.shape), xi.to(mag.dtype).reshape(mag.shape))
    return res + (part,) if part is not None else res


def _gl_convergence(parts):
    """conv[i, n] = sqrt(sum (|C| - S)^2 / sum S^2) from the stacked sums (n_iter, N, chunks, 2), added up in float64; 0 where S is 0"""
    sums = parts.double().sum(dim=2)
    num, den = sums[..., 0], sums[..., 1]
    return torch.where(den > 0, torch.sqrt(num / den.clamp_min(torch.finfo(torch.float64).tiny)), torch.zeros_like(den))


def griffinlim(mag, stft, n_iter=32, momentum=0.99, length=None, init_phase=None, rand_init=True, generator=None, frames=None,
               return_convergence=False):
    """a waveform whose STFT magnitude approaches `mag` (..., K, F), by the loop of include/psnd.h - torchaudio's functional.griffinlim,
    librosa's griffinlim (fast Griffin-Lim, Perraudin et al. 2013) - with `stft.transform_complex` / `stft.inverse_complex` as the two
    transforms (models.transforms.STFT): X0 from griffinlim_start, then `n_iter` times inverse, transform, griffinlim_step with
    alpha = momentum / (1 + momentum) and eps = 1e-16, then the inverse.  Returns (..., length or (F - 1) hop) in mag's dtype and on its
    device, trimmed or zero-padded; with `return_convergence` also conv (n_iter, N) float64, conv[i, n] = sqrt(sum (|C| - S)^2 / sum S^2)
    of iteration i.  `init_phase` (mag's shape) sets the first phase; else `rand_init` draws 2 pi torch.rand(...) once on mag's device
    (`generator`); else the phase is 0.  0 <= momentum < 1; n_iter >= 0, n_iter = 0 returns the inverse of X0.  `frames` as in
    griffinlim_start.

    On HIP tensors every iteration is three calls of the library and no library op: the two transforms and psnd_griffinlim_step, which
    writes X over the buffers of the spectrum of the iteration before; nothing synchronises with the host, so the loop can be captured.
    Off the iterated path and in library ops: the one draw of the random phase, and - with `return_convergence` - one float64 reduction
    of the per-chunk sums after the last iteration.  CPU tensors run the same loop through the host transforms in float64 and are cast
    back.  Runs under torch.no_grad(): no autograd, gradients through the loop are out of scope."""
    who = 'griffinlim'
    if not isinstance(mag, torch.Tensor):
        raise _lib.PsndError('%s: a tensor is expected, got %s' % (who, type(mag).__name__))
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
        raise ValueError('%s: n_iter=%r - an integer >= 0' % (who, n_iter))
    try:
        m = float(momentum)
    except (TypeError, ValueError):
        raise ValueError('%s: momentum=%r - a number in [0, 1)' % (who, momentum))
    if isinstance(momentum, bool) or not 0.0 <= m < 1.0:
        raise ValueError('%s: momentum=%r - a number in [0, 1)' % (who, momentum))
    if length is not None and (isinstance(length, bool) or not isinstance(length, int) or length < 0):
        raise ValueError('%s: length=%r - an integer >= 0 or None' % (who, length))
    lead, N, K, F, frames = _gl_planes(who, [('mag', mag), ('init_phase', init_phase)], frames)
    if K != stft.filter_length // 2 + 1:
        raise _lib.PsndError('%s: mag has %d bins, STFT(%d, %d) has %d' % (who, K, stft.filter_length, stft.hop_length, stft.filter_length // 2 + 1))
    hop = stft.hop_length
    if n_iter > 0 and (F - 1) * hop <= stft.filter_length // 2:
        raise _lib.PsndError('%s: %d frames give %d samples, the transform\'s reflect padding needs more than %d' % (
            who, F, max(F - 1, 0) * hop, stft.filter_length // 2))
    alpha = m / (1.0 + m)
    work = torch.float32 if mag.is_cuda else torch.float64
    with torch.no_grad():
        S = mag.detach().reshape(N, K, F).to(work).contiguous()
        if init_phase is not None:
            phi = init_phase.detach().reshape(N, K, F).to(work)
        elif rand_init:
            phi = ((2.0 * math.pi) * torch.rand((N, K, F), dtype=torch.float32, device=mag.device, generator=generator)).to(work)
        else:
            phi = None
        X = griffinlim_start(S, phi, frames)
        P, parts = None, []
        for _ in range(n_iter):
            C = stft.transform_complex(stft.inverse_complex(X[0], X[1]))
            C = (C[0].to(work), C[1].to(work))
            r = griffinlim_step(S, C[0], C[1], None if P is None else P[0], None if P is None else P[1], alpha, GL_EPS, frames,
                                out=P if mag.is_cuda else None, partial=return_convergence)
            X, P = r[:2], C
            if return_convergence:
                parts.append(r[2])
        y = stft.inverse_complex(X[0], X[1])
        n = (F - 1) * hop if length is None else length
        if y.shape[-1] >= n:
            y = y[..., :n].contiguous()
        else:
            y = torch.nn.functional.pad(y, (0, n - y.shape[-1]))
        y = y.to(mag.dtype).reshape(lead + (n,))
        if not return_convergence:
            return y
        conv = _gl_convergence(torch.stack(parts)) if parts else torch.zeros((0, N), dtype=torch.float64, device=mag.device)
    return y, conv


MEL_INVERSE_ITER_MAX = 256      # the momentum factors a plan is built with unless told otherwise


def mel_inverse_tile(M, K):
    """psnd_mel_inverse_tile: the consecutive frames of one item a workgroup of psnd_mel_inverse.hip owns - the size its seams depend on"""
    return int(lib().psnd_mel_inverse_tile(int(M), int(K)))


def _mi_filter(mel_filter, who):
    if isinstance(mel_filter, torch.Tensor):
        mel_filter = mel_filter.detach().cpu().numpy()
    W = np.array(mel_filter, dtype=np.float32, order='C')         # a copy: a plan is built lazily and must not follow later writes to the caller's array
    if W.ndim != 2 or W.size == 0:
        raise _lib.PsndError('%s: the filterbank must be a non-empty (M, K) matrix, got %s' % (who, W.shape))
    if not np.isfinite(W).all() or (W < 0).any():
        raise _lib.PsndError('%s: the filterbank must be finite and >= 0 (a negative or non-finite weight is an error, not a clamp)' % who)
    return W


def mel_inverse_plan_host(mel_filter, n_iter_max=MEL_INVERSE_ITER_MAX):
    """the plan of include/psnd.h's mel-inverse section in numpy: {A fp32 (M, K), d, cinv, c float64, L, step floats, beta fp32
    (n_iter_max,)}.  Every sum adds its terms one after the other in ascending index, as the C++ builder does: the two agree to the bit."""
    W = _mi_filter(mel_filter, 'mel_inverse_plan').astype(np.float64)
    M, K = W.shape
    s = np.zeros(M)
    for k in range(K):
        s = s + W[:, k]
    d = np.where(s > 0, 1.0 / np.where(s > 0, s, 1.0), 0.0)
    A = (d[:, None] * W).astype(np.float32)
    A64 = A.astype(np.float64)
    c = np.zeros(K)
    for m in range(M):
        c = c + A64[m]
    cinv = np.where(c > 0, 1.0 / np.where(c > 0, c, 1.0), 0.0)
    rows = np.zeros(M)
    for k in range(K):
        rows = rows + A64[:, k] * c[k]
    L = float(rows.max())
    beta, t = np.zeros(int(n_iter_max), dtype=np.float32), 1.0
    for i in range(int(n_iter_max)):
        tn = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        beta[i] = (t - 1.0) / tn
        t = tn
    return dict(A=A, d=d, cinv=cinv, c=c, L=L, step=1.0 / L if L > 0 else 0.0, beta=beta)


class MelInversePlan:
    """what mel_inverse needs of a filterbank (M, K): the numpy plan (A, d, cinv, step, beta: mel_inverse_plan_host) for CPU tensors and,
    built on first use through psnd_mel_inverse_plan_build and then kept per device, the table the kernel reads.  `raw()` is the C-built
    plan as a dict of views (the same names, plus d32, cinv32, step32 - what the kernel takes - and the band tables)."""

    def __init__(self, mel_filter, n_iter_max=MEL_INVERSE_ITER_MAX):
        if isinstance(n_iter_max, bool) or not isinstance(n_iter_max, int) or n_iter_max < 0:
            raise ValueError('mel_inverse_plan: n_iter_max=%r - an integer >= 0' % (n_iter_max,))
        self.W = _mi_filter(mel_filter, 'mel_inverse_plan')
        self.W.setflags(write=False)
        self.M, self.K = self.W.shape
        self.n_iter_max = n_iter_max
        self._np = None
        self._host = None
        self._dev = {}

    @property
    def host(self):
        if self._np is None:
            self._np = mel_inverse_plan_host(self.W, self.n_iter_max)
        return self._np

    def bytes(self):
        """the plan psnd_mel_inverse_plan_build writes, a numpy uint8 array (host)"""
        if self._host is None:
            nb = int(lib().psnd_mel_inverse_plan_bytes(self.M, self.K))
            if nb == 0:
                raise _lib.PsndError('mel_inverse_plan: M=%d K=%d: psnd_mel_inverse serves M <= 256 filters and K <= 2049 bins' % (self.M, self.K))
            plan = np.zeros(nb, dtype=np.uint8)
            check(lib().psnd_mel_inverse_plan_build(self.M, self.K, _lib.np_ptr(self.W), self.n_iter_max, _lib.np_ptr(plan)),
                  'psnd_mel_inverse_plan_build')
            self._host = plan
        return self._host

    def raw(self):
        w = self.bytes().view(np.uint32)
        M, K = int(w[1]), int(w[2])
        f64 = w[int(w[16]):int(w[16]) + 2 * (2 + M + K)].view(np.float64)
        f32 = lambda off, n: w[int(off):int(off) + n].view(np.float32)      # noqa: E731
        return dict(M=M, K=K, n_iter_max=int(w[3]), nnz_rows=int(w[4]), nnz_cols=int(w[5]), step32=float(w[6:7].view(np.float32)[0]),
                    d32=f32(w[8], M), cinv32=f32(w[9], K), beta=f32(w[10], int(w[3])), row_bands=w[int(w[11]):int(w[11]) + 2 * M].reshape(M, 2),
                    col_bands=w[int(w[12]):int(w[12]) + 2 * K].reshape(K, 2), row_weights=f32(w[13], int(w[4])), col_weights=f32(w[14], int(w[5])),
                    A=f32(w[15], M * K).reshape(M, K), step=float(f64[0]), L=float(f64[1]), d=f64[2:2 + M], cinv=f64[2 + M:2 + M + K])

    def tensor(self, device):
        """the plan on `device`; copied from the host once per device"""
        key = str(torch.device(device))
        t = self._dev.get(key)
        if t is None:
            t = self._dev[key] = plan_tensor(self.bytes()).to(device)
        return t

    def to(self, device):
        if torch.device(device).type == 'cuda':
            self.tensor(device)
        return self


def mel_inverse_plan(mel_filter, n_iter_max=MEL_INVERSE_ITER_MAX):
    """MelInversePlan of a filterbank (M, K), finite and >= 0 (PsndError otherwise), good for up to n_iter_max iterations"""
    return MelInversePlan(mel_filter, n_iter_max)


def _mi_plan(plan_or_filter, n_iter):
    if isinstance(plan_or_filter, MelInversePlan):
        return plan_or_filter
    return MelInversePlan(plan_or_filter, max(int(n_iter), 0))


def _mi_undo_log(Y, log_kind, log_offset):
    if log_kind == LOG_E:
        return np.exp(Y) - log_offset
    if log_kind == LOG_10:
        return np.power(10.0, Y) - log_offset
    if log_kind == LOG_NONE:
        return Y
    raise ValueError('mel_inverse: log_kind=%r' % (log_kind,))


def mel_inverse_host(mel, plan_or_filter, n_iter=64, log_kind=LOG_NONE, log_offset=0.0, frames=None, return_residual=False):
    """the mel-inverse section of include/psnd.h on a float64 numpy array (N, M, F): the definition, all frames at once - and the CPU
    path of mel_inverse.  Returns x (N, K, F) float64, with `return_residual` also |A x - b| / |b| per frame (N, F)."""
    if isinstance(n_iter, bool) or not isinstance(n_iter, (int, np.integer)) or n_iter < 0:
        raise ValueError('mel_inverse: n_iter=%r - an integer >= 0' % (n_iter,))
    plan = _mi_plan(plan_or_filter, n_iter)
    Y = np.asarray(mel, dtype=np.float64)
    if Y.ndim != 3 or Y.shape[1] != plan.M:
        raise ValueError('mel_inverse: (N, %d, F) expected, got %s' % (plan.M, Y.shape))
    if n_iter > plan.n_iter_max:
        raise ValueError('mel_inverse: n_iter=%d, the plan was built for %d' % (n_iter, plan.n_iter_max))
    N, _, F = Y.shape
    h = plan.host
    A, d, cinv, step, beta = h['A'].astype(np.float64), h['d'], h['cinv'], h['step'], h['beta']
    live = np.arange(F)[None, None, :] < _gl_host_frames(frames, N, F)[:, None, None]
    with np.errstate(invalid='ignore', over='ignore'):
        lin = _mi_undo_log(np.where(live, Y, 0.0), log_kind, float(log_offset))
        b = np.where(live, d[None, :, None] * np.maximum(lin, 0.0), 0.0)
        x = cinv[None, :, None] * np.einsum('mk,nmf->nkf', A, b)
        z = x
        for i in range(n_iter):
            r = np.einsum('mk,nkf->nmf', A, z) - b
            g = np.einsum('mk,nmf->nkf', A, r)
            xn = np.maximum(z - step * g, 0.0)
            z = xn + float(beta[i]) * (xn - x)
            x = xn
        x = np.where(live, x, 0.0)
        if not return_residual:
            return x
        r = np.einsum('mk,nkf->nmf', A, x) - b
        rr, bb = (r * r).sum(axis=1), (b * b).sum(axis=1)
        return x, np.where(bb > 0, np.sqrt(rr / np.where(bb > 0, bb, 1.0)), 0.0)


def mel_inverse(mel, plan_or_filter, n_iter=64, log_kind=LOG_NONE, log_offset=0.0, frames=None, return_residual=False):
    """a linear magnitude (..., K, F) >= 0 whose mel projection approaches `mel` (..., M, F), by the definition of include/psnd.h: per
    frame min_{x >= 0} |A x - b|^2 with the row-normalised filterbank A, `n_iter` FISTA steps from the flat-band guess (n_iter = 0 returns
    the guess).  `plan_or_filter`: a MelInversePlan (mel_inverse_plan - keeps the device table, nothing is copied from the host after its
    first use on a device) or the (M, K) filterbank itself, finite and >= 0 (a plan is then built in the call).  `log_kind`, `log_offset`:
    what `mel` is - linear (LOG_NONE), log(lin + offset) (LOG_E) or log10(lin + offset) (LOG_10).  `frames`: valid frames per item (one
    integer per leading index, clamped to [0, F]); what lies behind is never read and comes out 0.  `return_residual`: also
    |A x - b| / |b| per frame, (..., F), float32 on HIP tensors and float64 on CPU tensors.

    HIP tensors run psnd_mel_inverse (float32; float16 / bfloat16 are cast in and out; float64 raises; non-contiguous input is made
    contiguous): ONE launch for all iterations, no library op, no host synchronisation - the call can be captured.  CPU tensors go through
    mel_inverse_host in float64.  The result is in mel's dtype and on its device.  No autograd."""
    who = 'mel_inverse'
    if isinstance(n_iter, bool) or not isinstance(n_iter, int) or n_iter < 0:
        raise ValueError('%s: n_iter=%r - an integer >= 0' % (who, n_iter))
    if log_kind not in (LOG_NONE, LOG_E, LOG_10):
        raise ValueError('%s: log_kind=%r' % (who, log_kind))
    plan = _mi_plan(plan_or_filter, n_iter)
    lead, N, M, F, frames = _gl_planes(who, [('mel', mel)], frames)
    if M != plan.M:
        raise _lib.PsndError('%s: mel has %d bands, the filterbank %d' % (who, M, plan.M))
    if n_iter > plan.n_iter_max:
        raise _lib.PsndError('%s: n_iter=%d, the plan was built for %d (mel_inverse_plan(mel_filter, n_iter_max))' % (who, n_iter, plan.n_iter_max))
    Kb = plan.K
    if not mel.is_cuda:
        r = mel_inverse_host(mel.detach().reshape(N, M, F).to(torch.float64).numpy(), plan, n_iter, log_kind, log_offset,
                             None if frames is None else frames.numpy(), return_residual)
        x = torch.from_numpy(np.ascontiguousarray(r[0] if return_residual else r)).to(mel.dtype).reshape(lead + (Kb, F))
        return (x, torch.from_numpy(np.ascontiguousarray(r[1])).reshape(lead + (F,))) if return_residual else x
    Y = mel.detach().reshape(N, M, F).float().contiguous()
    out = torch.empty((N, Kb, F), dtype=torch.float32, device=mel.device)
    resid = torch.empty((N, F), dtype=torch.float32, device=mel.device) if return_residual else None
    if N * F > 0:
        table = plan.tensor(mel.device)
        with on(mel.device) as hip:
            hip.psnd_mel_inverse(Y, N, F, M, Kb, table, int(log_kind), float(log_offset), n_iter, frames, out, resid)
    x = out.to(mel.dtype).reshape(lead + (Kb, F))
    return (x, resid.reshape(lead + (F,))) if return_residual else x


def mel_to_wave(mel, plan_or_filter, stft, n_iter=64, gl_iter=32, momentum=0.99, log_kind=LOG_NONE, log_offset=0.0, length=None,
                rand_init=True, generator=None, frames=None):
    """mel (..., M, F) -> waveform (..., length or (F - 1) hop): mel_inverse (`n_iter` steps, one launch), then griffinlim (`gl_iter`
    iterations, `momentum`) on `stft` - two calls on device tensors, no library op on either iterated path, capturable with
    rand_init=False.  No autograd."""
    mag = mel_inverse(mel, plan_or_filter, n_iter, log_kind, log_offset, frames)
    return griffinlim(mag, stft, gl_iter, momentum, length, None, rand_init, generator, frames)


def volnorm_forward(wav, window, hop, inv_gain, out_len):
    """psnd_volnorm_fwd: wav (B, L) fp32 -> (out (B, out_len), std (hops,)), one workgroup per hop; out_len from sound.volnorm_layout"""
    _need_cuda(wav, 'wav')
    wav = wav.contiguous()
    B, L = wav.shape
    hops = (L - window + hop - 1) // hop
    out = torch.empty((B, out_len), dtype=torch.float32, device=wav.device)
    std = torch.empty(hops, dtype=torch.float32, device=wav.device)
    with on(wav.device) as hip:
        hip.psnd_volnorm_fwd(wav, B, L, int(window), int(hop), float(inv_gain), out, int(out_len), std)
    return out, std


def volnorm_reverse(wav, window, hop, gain, std, out_len):
    """psnd_volnorm_reverse: wav (B, L) fp32 and the hops' deviations std (>= hops,) on the device -> out (B, out_len)"""
    _need_cuda(wav, 'wav')
    _need_cuda(std, 'std')
    wav, std = wav.contiguous(), std.contiguous()
    B, L = wav.shape
    if std.numel() < (L - window + hop - 1) // hop:
        raise _lib.PsndError('volnorm_reverse: %d deviations for %d hops' % (std.numel(), (L - window + hop - 1) // hop))
    out = torch.empty((B, out_len), dtype=torch.float32, device=wav.device)
    with on(wav.device) as hip:
        hip.psnd_volnorm_reverse(wav, B, L, int(window), int(hop), float(gain), std, out, int(out_len))
    return out


def _msl_fused(n_fft, hop):
    """psnd_stft_bwd_msl takes this resolution (PSND_MSL_FUSED=0: the two-launch path, for A/B runs and tests)."""
    import os
    return (_sw.lab('PSND_MSL_FUSED', '1') != '0' and _mr_plan_bytes(int(n_fft)) == 0
            and bool(lib().psnd_stft_bwd_msl_supported(int(n_fft), int(hop))))


MSL_SIZES = 'powers of two in [16, 8192] and the multiples of 16 among the even 2^a 3^b 5^c up to 4096: 400, 480, 640, 800, 960, 1200, 1600, 2400 ...'


def msl_covered(n_fft):
    """multi_stft_loss takes this n_fft on a HIP tensor.  Narrower than stft_plan on purpose: the loss has always refused n_fft = 1000
    (8 * 125) and that refusal is part of its tested contract, so of the mixed-radix sizes it admits the multiples of 16 - every framing
    in use at 16 / 24 / 48 kHz but 600 and 1000."""
    n_fft = int(n_fft)
    if _mr_plan_bytes(n_fft) > 0:
        return n_fft % 16 == 0
    return int(lib().psnd_stft_plan_bytes(n_fft)) > 0


def msl_check(n_ffts):
    for n_fft in n_ffts:
        if not msl_covered(n_fft):
            raise _lib.PsndError('multi_stft_loss: n_fft=%d unsupported on a HIP tensor (%s)' % (n_fft, MSL_SIZES))


class MultiStftLossFn(torch.autograd.Function):
    """(loss, sc_loss, mag_loss) of sound.py:106-133 as ONE autograd node: per resolution two psnd_stft_fwd launches
    (pred, target) and one partial-sum pass, one combining launch for all resolutions; backward: per resolution one
    gradient pass over the magnitudes and psnd_stft_bwd, the waveform gradients of the resolutions added up.
    `cfgs`: tuple of (n_fft, hop) per resolution, `plans`: their device plans (window centre-padded to n_fft)."""

    @staticmethod
    def forward(ctx, pred, target, eps, cfgs, *plans):
        import ctypes
        _need_cuda(pred, 'pred')
        _need_cuda(target, 'target')
        if pred.shape != target.shape or pred.dim() != 2:
            raise _lib.PsndError('multi_stft_loss: pred %s and target %s must be equal (N, T) shapes'
                                 % (tuple(pred.shape), tuple(target.shape)))
        msl_check(n for n, _ in cfgs)
        pred, target = pred.contiguous(), target.contiguous()
        N = pred.shape[0]
        L = len(cfgs)
        dev = pred.device
        mags, parts, kfs, blocks = [], [], [], []
        # training case (only the prediction needs a gradient): the prediction's magnitudes never reach HBM - psnd_stft_fwd_msl leaves
        # the three sums, psnd_stft_bwd_msl recomputes |X| in the backward
        only_pred = not ctx.needs_input_grad[1]
        with on(dev) as hip:
            for (n_fft, hop), plan in zip(cfgs, plans):
                t = stft_forward(target, n_fft, hop, plan)['mag']
                KF = t.shape[1] * t.shape[2]
                B = int(lib().psnd_stft_fwd_msl_blocks(pred.shape[1], int(n_fft), int(hop))) if only_pred and _msl_fused(n_fft, hop) else 0
                if B > 0:
                    p = None
                    part = torch.empty((N, B, 3), dtype=torch.float64, device=dev)
                    hip.psnd_stft_fwd_msl(pred, N, pred.shape[1], int(n_fft), int(hop), plan, 0.0, t, float(eps), part)
                else:
                    p = stft_forward(pred, n_fft, hop, plan)['mag']
                    B = int(lib().psnd_stft_loss_blocks(KF))
                    part = torch.empty((N, B, 3), dtype=torch.float64, device=dev)
                    hip.psnd_stft_loss_partial(p, t, N, KF, float(eps), part)
                mags.append((p, t))
                parts.append(part)
                kfs.append(KF)
                blocks.append(B)
            norms = torch.empty((L, N, 2), dtype=torch.float32, device=dev)
            out = torch.empty(3, dtype=torch.float32, device=dev)
            parr = (ctypes.c_void_p * L)(*[q.data_ptr() for q in parts])
            karr = (ctypes.c_int64 * L)(*kfs)
            barr = (ctypes.c_int64 * L)(*blocks)
            hip.psnd_stft_loss_final_blocks(parr, karr, barr, L, N, norms, out)
        ctx.cfgs, ctx.eps, ctx.kfs = cfgs, float(eps), kfs
        ctx.has_p = [pt[0] is not None for pt in mags]
        ctx.save_for_backward(pred, target, norms, *[m if m is not None else norms for pt in mags for m in pt], *plans)
        return out

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        L = len(ctx.cfgs)
        pred, target, norms = saved[:3]
        mags, plans = saved[3:3 + 2 * L], saved[3 + 2 * L:]
        N = pred.shape[0]
        need_p, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = g.contiguous().float()
        gpred = gtarget = None
        with on(pred.device) as hip:
            for i, (n_fft, hop) in enumerate(ctx.cfgs):
                p, t = mags[2 * i], mags[2 * i + 1]
                if not ctx.has_p[i] or (need_p and not need_t and _msl_fused(n_fft, hop)):
                    # one launch: the adjoint STFT recomputes |X| and forms the loss gradient in registers (psnd_stft_bwd_msl)
                    # ... and adds it to the gradient of the resolutions before it (no memset, no add launch)
                    acc = gpred is not None
                    if not acc:
                        gpred = torch.empty_like(pred)
                    hip.psnd_stft_bwd_msl(pred, N, pred.shape[1], n_fft, hop, FRAMING_CENTER, plans[i], 0.0, t, norms[i], g, L, ctx.eps, int(acc),
                                          gpred)
                    continue
                gp = torch.empty_like(p) if need_p else None
                gt = torch.empty_like(t) if need_t else None
                hip.psnd_stft_loss_bwd(p, t, N, ctx.kfs[i], ctx.eps, norms[i], g, L, gp, gt)
                if need_p:
                    gw = stft_backward(pred, n_fft, hop, plans[i], gmag=gp)
                    gpred = gw if gpred is None else gpred.add_(gw)
                if need_t:
                    gw = stft_backward(target, n_fft, hop, plans[i], gmag=gt)
                    gtarget = gw if gtarget is None else gtarget.add_(gw)
        return (gpred, gtarget, None, None) + (None,) * L


# ---------------------------------------------------------------------------------------------
# PQMF (models/transforms.py:492-560): polyphase analysis / synthesis, each the other's adjoint with reversed taps
# ---------------------------------------------------------------------------------------------
def _pqmf(op, x, filt, subbands, taps, flip, scale, t_out=None):
    _need_cuda(x, 'input')
    x, filt = x.contiguous(), filt.contiguous()
    dev = x.device
    with on(dev) as hip:
        if op == 'analysis':                        # (B, T) -> (B, S, T // S)
            B, T = x.shape
            out = torch.empty((B, subbands, T // subbands), dtype=torch.float32, device=dev)
            hip.psnd_pqmf_analysis(x, filt, B, T, subbands, taps, int(flip), float(scale), out)
        else:                                       # (B, S, M) -> (B, M * S)
            B, S, M = x.shape
            t_out = M * S if t_out is None else t_out
            out = torch.empty((B, t_out), dtype=torch.float32, device=dev)
            hip.psnd_pqmf_synthesis(x, filt, B, M, t_out, subbands, taps, int(flip), float(scale), out)
    return out


class PqmfAnalysis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, filt, subbands, taps):
        ctx.save_for_backward(filt)
        ctx.cfg = (subbands, taps, x.shape[1])
        return _pqmf('analysis', x, filt, subbands, taps, 0, 1.0)

    @staticmethod
    def backward(ctx, g):
        (filt,) = ctx.saved_tensors
        S, taps, T = ctx.cfg
        return _pqmf('synthesis', g.contiguous(), filt, S, taps, 1, 1.0, t_out=T), None, None, None   # tail samples reach the last frames


class PqmfSynthesis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, filt, subbands, taps):
        ctx.save_for_backward(filt)
        ctx.cfg = (subbands, taps)
        return _pqmf('synthesis', x, filt, subbands, taps, 0, float(subbands))

    @staticmethod
    def backward(ctx, g):
        (filt,) = ctx.saved_tensors
        S, taps = ctx.cfg
        return _pqmf('analysis', g.contiguous(), filt, S, taps, 1, float(S)), None, None, None


class L1Loss(torch.autograd.Function):
    """F.l1_loss(a, b) (mean): one pass + a tiny combine forward, one pass backward (torch: sub, abs, mean / sign, scale, neg)."""

    @staticmethod
    def forward(ctx, a, b):
        _need_cuda(a, 'input')
        _need_cuda(b, 'target')
        if a.shape != b.shape:
            raise _lib.PsndError('l1_loss: shapes %s and %s differ' % (tuple(a.shape), tuple(b.shape)))
        a, b = a.contiguous(), b.contiguous()
        n = a.numel()
        part = torch.empty(int(lib().psnd_l1_loss_blocks(n)), dtype=torch.float64, device=a.device)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        with on(a.device) as hip:
            hip.psnd_l1_loss_fwd(a, b, n, part, out)
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        g = g.contiguous().float()
        with on(a.device) as hip:
            hip.psnd_l1_loss_bwd(a, b, a.numel(), g, ga, gb)
        return ga, gb


class L1LossSum(torch.autograd.Function):
    """sum_i w_i * F.l1_loss(a_i, b_i) as ONE scalar node (psnd_l1_loss_sum_fwd: one pass per term + one combine; backward one pass per
    term with the weight folded in) - a recipe's `l1(a, b) + 0.5 * l1(c, d)` without the scalar multiply / add launches."""

    @staticmethod
    def forward(ctx, weights, *tensors):
        import ctypes
        k = len(weights)
        if k < 1 or k > 4 or len(tensors) != 2 * k:
            raise _lib.PsndError('l1_loss_sum: 1 .. 4 (input, target) pairs with one weight each')
        ab = []
        for i in range(k):
            a, b = tensors[2 * i], tensors[2 * i + 1]
            _need_cuda(a, 'input')
            _need_cuda(b, 'target')
            if a.shape != b.shape:
                raise _lib.PsndError('l1_loss_sum: shapes %s and %s differ' % (tuple(a.shape), tuple(b.shape)))
            ab += [a.contiguous(), b.contiguous()]
        dev = ab[0].device
        ns = [ab[2 * i].numel() for i in range(k)]
        part = torch.empty(sum(int(lib().psnd_l1_loss_blocks(n)) for n in ns), dtype=torch.float64, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        pa = (ctypes.c_void_p * k)(*[ab[2 * i].data_ptr() for i in range(k)])
        pb = (ctypes.c_void_p * k)(*[ab[2 * i + 1].data_ptr() for i in range(k)])
        pn = (ctypes.c_int64 * k)(*ns)
        pw = (ctypes.c_double * k)(*[float(w) for w in weights])
        with on(dev) as hip:
            hip.psnd_l1_loss_sum_fwd(pa, pb, pn, pw, k, part, out)
        ctx.weights = tuple(float(w) for w in weights)
        ctx.save_for_backward(*ab)
        return out

    @staticmethod
    def backward(ctx, g):
        ab = ctx.saved_tensors
        g = g.contiguous().float()
        grads = []
        with on(g.device) as hip:
            for i, w in enumerate(ctx.weights):
                a, b = ab[2 * i], ab[2 * i + 1]
                ga = torch.empty_like(a) if ctx.needs_input_grad[1 + 2 * i] else None
                gb = torch.empty_like(b) if ctx.needs_input_grad[2 + 2 * i] else None
                if ga is not None or gb is not None:
                    hip.psnd_l1_loss_bwd_w(a, b, a.numel(), g, w, ga, gb)
                grads += [ga, gb]
        return (None,) + tuple(grads)


class MaskedL1(torch.autograd.Function):
    """sum |a - b| w / (C sum w) over (N, C, T) tensors with a per-frame weight w (N, T): the loss of a padded-batch recipe (clips of
    different lengths padded to the batch maximum, data/dataset.py:196-250) - psnd_masked_l1_fwd / _bwd instead of abs / mul / two sums /
    div and their autograd twins"""

    @staticmethod
    def forward(ctx, a, b, w):
        _need_cuda(a, 'input')
        _need_cuda(b, 'target')
        _need_cuda(w, 'frame weight')
        a, b, w = a.contiguous(), b.contiguous(), w.contiguous()
        N, C, T = a.shape
        if b.shape != a.shape or tuple(w.shape) != (N, T):
            raise _lib.PsndError('masked_l1_loss: input %s, target %s, frame weight %s' % (tuple(a.shape), tuple(b.shape), tuple(w.shape)))
        part = torch.empty(2 * int(lib().psnd_masked_l1_blocks(a.numel())), dtype=torch.float64, device=a.device)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        inv = torch.empty(1, dtype=torch.float32, device=a.device)
        with on(a.device) as hip:
            hip.psnd_masked_l1_fwd(a, b, w, N, C, T, part, out, inv)
        ctx.save_for_backward(a, b, w, inv)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b, w, inv = ctx.saved_tensors
        N, C, T = a.shape
        g = g.contiguous().float()
        ga = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        gb = torch.empty_like(b) if ctx.needs_input_grad[1] else None
        if ga is None and gb is None:
            return None, None, None
        with on(a.device) as hip:
            hip.psnd_masked_l1_bwd(a, b, w, N, C, T, g, inv, ga, gb)
        return ga, gb, None


def masked_l1_loss(input, target, frame_weight):
    """sum |input - target| * frame_weight[:, None, :] / (C * frame_weight.sum()) on fp32 HIP tensors (N, C, T) / (N, T)"""
    return MaskedL1.apply(input, target, frame_weight)


def l1_loss_sum(pairs, weights):
    """sum_i weights[i] * F.l1_loss(*pairs[i]) on fp32 HIP tensors, one autograd node"""
    flat = [t for p in pairs for t in p]
    return L1LossSum.apply(tuple(weights), *flat)


def l1_loss(input, target):
    """drop-in for torch.nn.functional.l1_loss(input, target) (reduction 'mean') on fp32 HIP tensors"""
    return L1Loss.apply(input, target)


# ---------------------------------------------------------------------------------------------
# LearnableSTFT (models/transforms.py:104-203): analysis / synthesis with trainable bases (psnd_lstft_*)
# ---------------------------------------------------------------------------------------------
def _lstft_basis(basis, window):
    b = basis.reshape(basis.shape[0], basis.shape[-1])
    _need_cuda(b, 'basis')
    _need_cuda(window, 'window')
    if window.numel() != b.shape[1]:
        raise PsndError('lstft: a window of %d taps for a basis %s' % (window.numel(), tuple(basis.shape)))
    return b.contiguous(), window.contiguous()


def lstft_analysis(x, basis, window, hop, polar=False):
    """spec[z][c][f] = sum_m basis[c][m] window[m] x[z][f hop + m] of a padded waveform x (N, Lx) - F.conv1d(x[:, None], (basis * window),
    stride=hop) without frames in memory.  Returns spec (N, C, F), and with `polar` also mag, phase (N, C / 2, F)."""
    _need_cuda(x, 'x')
    b, w = _lstft_basis(basis, window)
    x = x.contiguous()
    (N, Lx), (C, n) = x.shape, b.shape
    F = (Lx - n) // hop + 1 if hop > 0 and Lx >= n else 0
    spec = torch.empty((N, C, max(F, 0)), dtype=torch.float32, device=x.device)
    mag = torch.empty((N, C // 2, max(F, 0)), dtype=torch.float32, device=x.device) if polar else None
    phase = torch.empty_like(mag) if polar else None
    with on(x.device) as hip:
        hip.psnd_lstft_analysis(x, b, w, N, Lx, C, n, int(hop), spec, mag, phase)
    return (spec, mag, phase) if polar else spec


def lstft_synthesis(g, basis, window, hop, mult=None, length=None):
    """y[z][s] = mult[s] * sum_{c, f} g[z][c][f] basis[c][s - f hop] window[s - f hop] - F.conv_transpose1d(g, (basis * window)[:, None],
    stride=hop) in gather form (every sample written once).  g (N, C, F) -> y (N, length), length >= n + hop (F - 1) (default: equal)."""
    _need_cuda(g, 'g')
    b, w = _lstft_basis(basis, window)
    g = g.contiguous()
    (N, C, F), n = g.shape, b.shape[1]
    if C != b.shape[0]:
        raise PsndError('lstft_synthesis: %d rows for a basis %s' % (C, tuple(basis.shape)))
    L = n + hop * (F - 1) if length is None else int(length)
    if mult is not None:
        _need_cuda(mult, 'mult')
        if mult.numel() != L:
            raise PsndError('lstft_synthesis: a multiplier of %d samples for rows of %d' % (mult.numel(), L))
        mult = mult.contiguous()
    y = torch.empty((N, L), dtype=torch.float32, device=g.device)
    with on(g.device) as hip:
        hip.psnd_lstft_synthesis(g, b, w, mult, N, C, F, n, int(hop), L, y)
    return y


def lstft_basis_grad(g, x, window, hop, like):
    """gb[c][m] = window[m] * sum_{z, f} g[z][c][f] x[z][f hop + m] in the shape of `like` (the basis); slabs added in a fixed order"""
    _need_cuda(g, 'g')
    _need_cuda(x, 'x')
    g, x, w = g.contiguous(), x.contiguous(), window.contiguous()
    (N, C, F), Lx, n = g.shape, x.shape[1], w.numel()
    slabs = int(lib().psnd_lstft_wgrad_slabs(N, C, n, F))
    part = torch.empty((max(slabs, 1), C, n), dtype=torch.float32, device=g.device)
    gb = torch.empty((C, n), dtype=torch.float32, device=g.device)
    with on(g.device) as hip:
        hip.psnd_lstft_basis_grad(g, x, w, N, Lx, C, n, int(hop), F, part, gb)
    return gb.view(like.shape)


class LstftAnalysis(torch.autograd.Function):
    """LearnableSTFT.transform behind the reflect padding: x (N, Lx) -> mag, phase (N, C / 2, F).  phase carries no gradient (the
    reference takes it from `.data`).  Backward: gspec = gmag [re; im] / mag (NaN at a bin that is exactly zero, as autograd of sqrt and
    STFT.transform's backward give), waveform gradient = the synthesis operator with the same basis, basis gradient = psnd_lstft_basis_grad;
    either is skipped when it is not required."""

    @staticmethod
    def forward(ctx, x, basis, window, hop):
        spec, mag, phase = lstft_analysis(x, basis, window, hop, polar=True)
        ctx.save_for_backward(x, basis, window, spec, mag)
        ctx.hop = hop
        ctx.mark_non_differentiable(phase)
        return mag, phase

    @staticmethod
    def backward(ctx, gmag, _gphase):
        x, basis, window, spec, mag = ctx.saved_tensors
        gx = gb = None
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None
        gmag = gmag.contiguous().float()
        N, C, F = spec.shape
        gspec = torch.empty_like(spec)
        with on(x.device) as hip:
            hip.psnd_lstft_mag_bwd(spec, mag, gmag, N, C, F, gspec)
        if ctx.needs_input_grad[0]:
            gx = lstft_synthesis(gspec, basis, window, ctx.hop, None, x.shape[1])
        if ctx.needs_input_grad[1]:
            gb = lstft_basis_grad(gspec, x, window, ctx.hop, basis)
        return gx, gb, None, None


class LstftSynthesis(torch.autograd.Function):
    """LearnableSTFT.inverse between the polar -> (re, im) element ops and the final cut: spec (N, C, F) -> y (N, n + hop (F - 1)) times the
    per-sample multiplier `mult` (envelope division and n / hop scale).  Backward: input gradient = the analysis operator with the same
    basis on mult * gy, basis gradient = psnd_lstft_basis_grad with the roles of spectrum and waveform swapped."""

    @staticmethod
    def forward(ctx, spec, basis, window, mult, hop):
        y = lstft_synthesis(spec, basis, window, hop, mult)
        ctx.save_for_backward(spec, basis, window, mult)
        ctx.hop = hop
        return y

    @staticmethod
    def backward(ctx, gy):
        spec, basis, window, mult = ctx.saved_tensors
        gs = gb = None
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None
        gy = gy.contiguous().float()
        if mult is not None:
            gy = gy * mult
        if ctx.needs_input_grad[0]:
            gs = lstft_analysis(gy, basis, window, ctx.hop)
        if ctx.needs_input_grad[1]:
            gb = lstft_basis_grad(spec, gy, window, ctx.hop, basis)
        return gs, gb, None, None, None
