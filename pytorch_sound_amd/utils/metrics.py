"""Waveform-domain scores for enhancement and source separation: SNR, scale-invariant SDR and scale-dependent SDR (Le Roux et al., "SDR -
half-baked or well done?") and permutation-invariant matching.  The reference names the tasks - VoiceBank, DSD100 / MUSDB18 / MedleyDB -
and has no such function, so there is no parity to pin; the definition is the separation section of include/psnd.h, and the defaults
(`zero_mean`, eps = float32 machine epsilon) are torchmetrics'.

    snr, si_sdr, sd_sdr     dB per row of (..., T)
    pit                     the values under the best assignment of S estimates to S targets, and the assignment
    permute_sources         reorder sources by such an assignment

numpy in -> numpy out, tensor in -> tensor on the same device out.  On HIP tensors the moments of all rows of an item are taken in one
read by psnd_separation.hip (fp64 sums in a fixed order, so a residual 60 dB down is not lost in a difference of fp32 sums), nothing is
read back by the host, the calls can be captured, and the values carry a gradient to both inputs; numpy arrays and CPU tensors run the
same definition in float64 (`kernels.sep_metric_host`), without a gradient.  As a training loss use `models.sound.SeparationLoss`.

Not covered: BSS-eval SDR with a distortion filter (mir_eval, torchmetrics' signal_distortion_ratio), PESQ / STOI, Hungarian matching
for many sources (the search is over all S! permutations, S <= 4 on HIP tensors), multichannel items.
"""
import numpy as np

from .. import kernels


def _is_tensor(x):
    import torch
    return isinstance(x, torch.Tensor)


def _per_row(kind, est, target, zero_mean, lengths):
    if tuple(est.shape) != tuple(target.shape) or len(est.shape) < 1:
        raise kernels.PsndError('%s: estimate and target (..., T) of one shape expected, got %s and %s'
                                % (kind, tuple(est.shape), tuple(target.shape)))
    lead, T = tuple(est.shape[:-1]), est.shape[-1]
    if lengths is not None and _is_tensor(lengths):
        lengths = lengths.reshape(-1)
    elif lengths is not None:
        lengths = np.asarray(lengths).reshape(-1)
    v = kernels.sep_metric(est.reshape(-1, 1, T), target.reshape(-1, 1, T), kind, zero_mean, None, lengths)
    return v.reshape(lead)


def snr(est, target, zero_mean=False, lengths=None):
    """10 log10(|s|^2 / |s - e|^2) per row of (..., T) in dB, float32 of the leading shape; `lengths`: per-row valid lengths"""
    return _per_row('snr', est, target, zero_mean, lengths)


def si_sdr(est, target, zero_mean=True, lengths=None):
    """scale-invariant SDR per row in dB: the target scaled by a = <e, s> / |s|^2 against what is left of the estimate"""
    return _per_row('si_sdr', est, target, zero_mean, lengths)


def sd_sdr(est, target, zero_mean=False, lengths=None):
    """scale-dependent SDR per row in dB: the scaled target of `si_sdr` against the unscaled residual s - e"""
    return _per_row('sd_sdr', est, target, zero_mean, lengths)


def pit(est, target, kind='si_sdr', zero_mean=None, lengths=None, eps=None):
    """permutation-invariant matching of S estimates with S targets per item, `est` and `target` (..., S, T): (values, perm) - float32
    values (..., S) in dB of estimate i against target perm[..., i] under the permutation that maximises their sum (ties to the
    lexicographically first), and that int32 permutation.  `zero_mean` defaults to True for 'si_sdr' and False otherwise; `lengths` per
    item.  `permute_sources(target, perm)` lines the targets up with the estimates."""
    if zero_mean is None:
        zero_mean = kind == 'si_sdr'
    return kernels.sep_metric(est, target, kind, zero_mean, eps, lengths, pit=True, return_perm=True)


def permute_sources(x, perm):
    """y[..., i, :] = x[..., perm[..., i], :] for x (..., S, T) and perm (..., S): a gather along the source axis"""
    if _is_tensor(x):
        import torch
        idx = torch.as_tensor(perm, device=x.device).long()
        return torch.gather(x, -2, idx.unsqueeze(-1).expand(x.shape))
    return np.take_along_axis(np.asarray(x), np.broadcast_to(np.asarray(perm, dtype=np.int64)[..., None], np.shape(x)), axis=-2)
