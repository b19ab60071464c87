/*
 * psnd.h - C ABI of libpsnd_hip.so, the MI355X (gfx950) native hot path of pytorch_sound.
 *
 * The reference (AppleHolic/pytorch_sound, /root/reference) is pure Python: it has no FFI
 * for this path; every "kernel" there is an ATen call.  This header is therefore the binding
 * a maintainer adds (ctypes stub in INTEGRATION.md); each entry point cites the reference
 * lines whose arithmetic it replaces.
 *
 * Conventions (all entry points):
 *   - extern "C", plain pointers and sizes, no torch types.
 *   - device pointers unless the name says _host; caller owns every buffer, guarantees
 *     contiguity and 4-byte alignment (16-byte where noted) and lifetime until the stream
 *     has completed the work.
 *   - work is ENQUEUED on `stream` (a hipStream_t passed as void*); no entry point
 *     synchronises the device, allocates device memory or keeps mutable global state.
 *   - return 0 on success, a negative PSND_E_* otherwise; psnd_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - "plans" are small read-only tables (window, twiddles, filterbank bands) built on the
 *     HOST by psnd_*_plan_build into caller memory; the caller uploads them once to the
 *     device and passes the device copy to the compute entry points.
 */
#ifndef PSND_H
#define PSND_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSND_OK 0
#define PSND_E_ARG (-1)         /* null pointer / bad enum / unsupported size            */
#define PSND_E_SHAPE (-2)       /* shapes inconsistent (e.g. T <= pad, K != n_fft/2+1)    */
#define PSND_E_HIP (-3)         /* HIP runtime reported an error at enqueue time         */
#define PSND_E_UNSUPPORTED (-4) /* valid request the library has no kernel for (yet)     */

/* framing conventions */
#define PSND_FRAMING_CENTER 0  /* reflect-pad n_fft/2       : transforms.py:55-60, :298-301   */
#define PSND_FRAMING_HIFIGAN 1 /* reflect-pad (n_fft-hop)/2 : transforms.py:352-353,
                                  interface/hifi_gan.py:37,49 */
#define PSND_FRAMING_NONE 2    /* no padding: frame f covers samples [f*hop, f*hop + n_fft)  (used by the
                                  backward of psnd_istft)                                          */

int psnd_version(void);
const char *psnd_last_error(void);
#ifdef PSND_LAB
/* LAB builds only (libpsnd_hip_lab.so, `python -m pytorch_sound_amd._build --lab`): the dispatchers read PSND_* A/B switches (kernel-instance
 * choices, ablations, trace pointers) from the environment once per call site; a process that changes its environment afterwards (parity
 * tests flipping kernel instances) calls this to have them looked up again.  The product library has no environment switch. */
void psnd_env_refresh(void);
#endif

/* ---- stream events: release points inside a captured step graph (data-parallel training) ------------------------
 * psnd_event_record_external on a CAPTURING stream adds an external event-record node (hipEventRecordExternal): after the
 * graph launch, psnd_stream_wait_event(other_stream, ev) makes `other_stream` wait for that node of that launch only - the
 * gradient all-reduce of a bucket starts while the rest of the replayed backward still runs.  Outside a capture it is a plain
 * event record.  The reference has no distributed code; north_star: "all-reduce overlapped with backward". */
void *psnd_event_create(void);                 /* NULL on failure (psnd_last_error) */
int psnd_event_destroy(void *ev);
int psnd_event_record_external(void *ev, void *stream);
int psnd_stream_wait_event(void *stream, void *ev);
int psnd_event_external_supported(void);      /* 1: this HIP runtime captures external event-record nodes (probed once) */

/* ---- integer contract: frame indexing (bit-exact) -------------------------------------- */
/* number of frames of the strided conv over the reflect-padded signal
 * (transforms.py:55-66; F = T/hop + 1 for CENTER, T/hop for HIFIGAN when hop | T). */
int64_t psnd_frame_count(int64_t T, int n_fft, int hop, int framing);
/* original-sample index read by tap m of frame f (reflect map x[-i]=x[i], x[T-1+i]=x[T-1-i]). */
int64_t psnd_frame_sample_index(int64_t f, int m, int64_t T, int n_fft, int hop, int framing);

/* ---- STFT plan ------------------------------------------------------------------------- */
/* bytes of the plan for an n_fft-point transform (0 if n_fft unsupported). */
size_t psnd_stft_plan_bytes(int n_fft);
/* window_host: n_fft taps, already zero-centre-padded from win_length (transforms.py:30-32).
 * Fills plan_host (psnd_stft_plan_bytes(n_fft) bytes). */
int psnd_stft_plan_build(int n_fft, const float *window_host, void *plan_host);

/* ---- STFT forward: replaces STFT.transform (transforms.py:53-69),
 *      STFTTorchAudio.forward/transform (transforms.py:297-311), the torch.stft + sqrt of
 *      Audio2Mel.forward (transforms.py:351-363) and interface MelSpectrogram (hifi_gan.py:46-55).
 *   wav   : (N,T) fp32
 *   mag   : (N,K,F) fp32 or NULL     = sqrt(re^2 + im^2 + mag_eps)
 *   phase : (N,K,F) fp32 or NULL     = atan2(im, re)
 *   re,im : (N,K,F) fp32 or NULL (both or neither)
 *   K = n_fft/2+1, F = psnd_frame_count(T, n_fft, hop, framing); frame axis fastest. */
int psnd_stft_fwd(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing,
                  const void *plan, float mag_eps,
                  float *mag, float *phase, float *re, float *im, void *stream);

/* psnd_stft_fwd (magnitude only) with the BIN axis fastest: mag_nfk : (N,F,K) fp32 = the transpose of psnd_stft_fwd's mag over its last
 * two axes, same values.  transforms.py:53-69 fixes (N,K,F) at the module boundary (STFT.transform returns that); every consumer INSIDE
 * this library (psnd_mel_*, the channels-last conv stack, the spectral losses) can take either layout, and in this one a frame's spectrum
 * is one contiguous 4K-byte run: a wave stores whole cache lines that it owns alone.  Same algorithmic bytes (4NT + 4NKF).  Tuned
 * kernels for n_fft 1024 and 4096, the one-frame-per-workgroup kernel for every other supported size. */
int psnd_stft_mag_nfk(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing,
                      const void *plan, float mag_eps, float *mag_nfk, void *stream);

/* ---- STFT backward (autograd through transforms.py:55-69 / torch.stft):
 *   gwav[n,t] = sum over (f,m) with frame_sample_index(f,m)==t of
 *               win[m] * sum_k ( gre[n,k,f] cos(2 pi k m/n) - gim[n,k,f] sin(2 pi k m/n) )
 *   where, when gmag != NULL, gre += gmag*re/mag, gim += gmag*im/mag with re/im/mag recomputed
 *   from wav (mag = sqrt(re^2+im^2+mag_eps); 0/0 -> NaN exactly as autograd of sqrt does).
 *   gmag / gre / gim: (N,K,F) or NULL (gre and gim both or neither; at least one source).
 *   gwav : (N,T) fp32, fully overwritten. */
int psnd_stft_bwd(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing,
                  const void *plan, float mag_eps,
                  const float *gmag, const float *gre, const float *gim,
                  float *gwav, void *stream);

/* ---- gradient of STFTTorchAudio.transform (transforms.py:305-311: magnitude AND a differentiable atan2 phase):
 *      (g_mag, g_phase | mag, phase) -> (g_re, g_im), all (N,K,F) fp32 = n elements; either of g_mag / g_phase may be NULL.
 *      The result is what psnd_stft_bwd takes as gre / gim. */
int psnd_polar_bwd(const float *gmag, const float *gphase, const float *mag, const float *phase, int64_t n,
                   float *gre, float *gim, void *stream);

/* ---- inverse STFT: replaces STFT.inverse (transforms.py:71-101): per frame (hop/n) * window * irDFT(mag e^{i phase})
 *      (what the pinv synthesis basis computes), overlap-add, divide by the squared-window envelope + eps,
 *      scale n/hop, trim n/2 on both sides.   mag, phase : (N,K,F);  out : (N, (F-1)*hop) fp32, fully overwritten. */
int psnd_istft(const float *mag, const float *phase, int64_t N, int64_t F, int n_fft, int hop,
               const void *plan, float eps, float *out, void *stream);

/* ---- mixed-radix STFT: the three transforms above for the n_fft the power-of-two kernels leave out -----------------------------
 *  Covered: even n_fft = 2^a 3^b 5^c in [16, 4096] that is no power of two (400, 480, 600, 800, 960, 1200, 2400, 4000 ...: what
 *  STFTTorchAudio / Audio2Mel / LogMelSpectrogramTorchAudio / interface MelSpectrogram / multi_stft_loss meet at speech sample rates,
 *  transforms.py:271-366, sound.py:89-133).  Powers of two stay with psnd_stft_* (psnd_stft_plan_bytes(1000) is still 0).
 *
 *  Plan (psnd_stft_mr_plan_bytes(n_fft) = 4 (16 + 3 n_fft) bytes, 0 for an uncovered size), in 4-byte words:
 *    [0, 16)            int32 header: magic 0x3152464d, n_fft, P = number of passes, radix[0 .. P) in execution order - every factor 5,
 *                       then every 3, then every 4, then one 2 if a factor two is left (the product is n_fft) - zeros behind
 *    [16, 16 + n)       the window, n_fft fp32 taps as given (already centre-padded)
 *    [16 + n, 16 + 3n)  (cos, -sin)(2 pi j / n_fft), j < n_fft, computed in float64, one fp32 pair each
 *  The compute entry points take the device copy and its size: plan_bytes must equal psnd_stft_mr_plan_bytes(n_fft) (PSND_E_ARG - this
 *  is how a plan of the other kind or of another size is told apart without reading device memory).
 *
 *  psnd_stft_mr_fwd: psnd_stft_fwd's contract - three framings, mag_eps inside the square root, any subset of mag / phase / (re, im),
 *      each (N, K, F) fp32 fully overwritten; the reflect padding is index arithmetic, rows of wav need 4-byte alignment only.
 *  psnd_stft_mr_bwd: psnd_stft_bwd's contract (gmag and / or (gre, gim) -> gwav (N, T), fully overwritten; a bin with mag == 0 and
 *      mag_eps == 0 gives NaN as there).  Two launches and no float atomic: window * adjoint DFT of every frame goes to `scratch`
 *      (psnd_stft_mr_bwd_scratch_bytes(N, T, n_fft, hop, framing) bytes = 4 N F n_fft, device memory the caller provides), then every
 *      sample of gwav adds up the frame taps that read it - the sample itself, its left and its right mirror image under the reflect
 *      padding, frames ascending - so the result is bit-reproducible.
 *  psnd_istft_mr: psnd_istft's definition (windowed inverse real DFT of mag e^{i phase}, the imaginary parts of DC and Nyquist dropped,
 *      overlap-add, divided by the squared-window envelope + eps, n_fft / 2 trimmed on both sides; out (N, (F - 1) hop) fully overwritten;
 *      eps = 0 is torch.istft's convention) with the same two launches; psnd_istft_mr_scratch_bytes(N, F, n_fft) = 4 N F n_fft.
 *
 *  PSND_E_ARG without touching the device: a NULL required pointer, hop <= 0, a bad framing, plan_bytes of another plan, a scratch that is
 *  NULL or too small; PSND_E_SHAPE: T <= the reflect pad, index ranges beyond 2^31, N > 65535; PSND_E_UNSUPPORTED: an uncovered n_fft. */
size_t psnd_stft_mr_plan_bytes(int n_fft);
int psnd_stft_mr_plan_build(int n_fft, const float *window_host, void *plan_host);
int psnd_stft_mr_fwd(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing, const void *plan, size_t plan_bytes,
                     float mag_eps, float *mag, float *phase, float *re, float *im, void *stream);
size_t psnd_stft_mr_bwd_scratch_bytes(int64_t N, int64_t T, int n_fft, int hop, int framing);
int psnd_stft_mr_bwd(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing, const void *plan, size_t plan_bytes,
                     float mag_eps, const float *gmag, const float *gre, const float *gim, void *scratch, size_t scratch_bytes,
                     float *gwav, void *stream);
size_t psnd_istft_mr_scratch_bytes(int64_t N, int64_t F, int n_fft);
int psnd_istft_mr(const float *mag, const float *phase, int64_t N, int64_t F, int n_fft, int hop, const void *plan, size_t plan_bytes,
                  float eps, void *scratch, size_t scratch_bytes, float *out, void *stream);

/* ---- masked inverse STFT on (re, im): separator to waveform, both directions ----------------------------------------------------
 *  Forward: psnd_istft's definition applied to the spectrum S = m (re + i im) - per frame window * irDFT(S_f), the imaginary parts of
 *  the DC and Nyquist bins dropped, overlap-add, divided by env[t] + eps (env[t] = sum_f window^2[t - f hop]), n_fft / 2 trimmed on
 *  both sides; out (N, (F - 1) hop) fp32, fully overwritten.  eps = 0 is torch.istft's convention, 1e-9 STFT.inverse's.
 *    re, im : (N, K, F) fp32;  mask : (N, K, F) fp32 or NULL;  m by mask_kind: PSND_MASK_NONE 1 (mask must be NULL), PSND_MASK_LINEAR
 *    the mask, PSND_MASK_SIGMOID 1 / (1 + e^{-mask}) evaluated in the kernel (mask must not be NULL for the two).  mask * |X| e^{i arg X}
 *    is mask * X: no magnitude, no phase, no sin / cos between the mixture and the output.
 *  psnd_istft_reim: the power-of-two plans - a loader mode of psnd_istft's three kernel families, same dispatch, grid limits and errors.
 *      The output is zeroed by a kernel launch of its own (not a memset node), so a hipGraph capture replays it as it ran.
 *  psnd_istft_reim_mr: the mixed-radix plans - psnd_istft_mr's contract (plan_bytes, scratch of psnd_istft_mr_scratch_bytes, two
 *      launches, no float atomic).
 *  psnd_istft_reim_bwd: gradients for g = d loss / d out, (N, (F - 1) hop), either plan kind (told apart by n_fft; plan_bytes must be that
 *      plan's size), three launches on the caller's stream, no allocation, no synchronisation:
 *        1. gp[t] = g[t - p] / (env[t] + eps) for p <= t < L - p (p = n_fft / 2, L = (F - 1) hop + n_fft), 0 outside and where the
 *           denominator is 0; env from the plan's window, at most ceil(n_fft / hop) taps, frames ascending, no atomics
 *        2. A = psnd_stft_fwd / psnd_stft_mr_fwd of gp with PSND_FRAMING_NONE -> scratch
 *        3. are = s_k Re A, aim = s_k Im A (s_k = 1 / n_fft at DC and Nyquist, 2 / n_fft elsewhere; aim = 0 at DC and Nyquist);
 *           g_re = m are, g_im = m aim, g_m = re are + im aim; g_mask = g_m (LINEAR) or g_m sigma (1 - sigma) (SIGMOID, sigma
 *           recomputed from the logits)
 *      g_re and g_im: both or neither; g_mask: only with a mask; at least one output.  hop <= n_fft.
 *      psnd_istft_reim_bwd_scratch_bytes(N, F, n_fft) = 4 (r4(N F n_fft) + 2 r4(N K F)) with r4 = rounded up to a multiple of 4
 *      (0 for N <= 0, F <= 1 or an uncovered n_fft).
 *  PSND_E_ARG: a NULL required pointer, a mask pointer that does not agree with mask_kind, a bad mask_kind, plan_bytes of another
 *  plan, a scratch that is NULL or too small; PSND_E_UNSUPPORTED: an uncovered n_fft; N = 0 or F <= 1: PSND_OK, nothing launched. */
#define PSND_MASK_NONE 0
#define PSND_MASK_LINEAR 1
#define PSND_MASK_SIGMOID 2
int psnd_istft_reim(const float *re, const float *im, const float *mask, int mask_kind, int64_t N, int64_t F, int n_fft, int hop,
                    const void *plan, float eps, float *out, void *stream);
int psnd_istft_reim_mr(const float *re, const float *im, const float *mask, int mask_kind, int64_t N, int64_t F, int n_fft, int hop,
                       const void *plan, size_t plan_bytes, float eps, void *scratch, size_t scratch_bytes, float *out, void *stream);
size_t psnd_istft_reim_bwd_scratch_bytes(int64_t N, int64_t F, int n_fft);
int psnd_istft_reim_bwd(const float *g, const float *re, const float *im, const float *mask, int mask_kind, int64_t N, int64_t F,
                        int n_fft, int hop, const void *plan, size_t plan_bytes, float eps, void *scratch, size_t scratch_bytes,
                        float *g_re, float *g_im, float *g_mask, void *stream);

/* ---- mel projection + log + clamp: replaces transforms.py:235-243, :364-365,
 *      interface/hifi_gan.py:58-61 -------------------------------------------------------- */
#define PSND_LOG_NONE 0  /* linear mel                                   */
#define PSND_LOG_E 1     /* ln                                           */
#define PSND_LOG_10 2    /* log10                                        */
size_t psnd_mel_plan_bytes(int M, int K);
/* mel_filter_host: (M,K) fp32 row-major (the module's `mel_filter` buffer). */
int psnd_mel_plan_build(int M, int K, const float *mel_filter_host, void *plan_host);
/*   mag     : (N,K,F) fp32
 *   out     : (N,M,F) fp32 = clamp( log( max(mel, pre_clamp_min) + log_offset ), lo, hi )
 *             pre_clamp_min < 0 disables the inner max; lo/hi: pass -INF/+INF to disable.
 *   mel_lin : (N,M,F) fp32 or NULL - the un-logged product, saved for backward. */
int psnd_mel_fwd(const float *mag, int64_t N, int64_t F, int M, int K, const void *mel_plan,
                 int log_kind, float log_offset, float pre_clamp_min, float clamp_lo, float clamp_hi,
                 float *out, float *mel_lin, void *stream);
/*   gmag[n,k,f] = sum_m W[m,k] * gout[n,m,f] * dlog(mel_lin[n,m,f]) (0 where a clamp is active) */
int psnd_mel_bwd(const float *gout, const float *mel_lin, int64_t N, int64_t F, int M, int K,
                 const void *mel_plan, int log_kind, float log_offset, float pre_clamp_min,
                 float clamp_lo, float clamp_hi, float *gmag, void *stream);

/* Fused wav -> log-mel: psnd_stft_fwd (magnitude) + psnd_mel_fwd in ONE kernel - the (N,K,F) magnitude lives only in
 * LDS.  Forward only (LogMelSpectrogram.forward transforms.py:229-244 discards the magnitude and the phase; Audio2Mel
 * :351-366; interface/hifi_gan.py:46-63).  Covers n_fft = 1024, hop <= 256, hop % 4 == 0 (PSND_E_UNSUPPORTED otherwise:
 * call the two functions above).  Arguments as in psnd_stft_fwd / psnd_mel_fwd; out : (N,M,F) fp32. */
int psnd_logmel_fwd(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing, const void *stft_plan,
                    float mag_eps, int M, const void *mel_plan, int log_kind, float log_offset, float pre_clamp_min,
                    float clamp_lo, float clamp_hi, float *out, void *stream);

/* ---- Conv1d stacks of models/vocoders/hifi_gan.py:32-147 on channels-last bf16 ("CL") matrices -------------
 *  CL buffer: (N, Lp, Cp) bf16, row r = clip*Lp + l; rows l in [HP, HP+L) hold the clip, every other row is
 *  zero (they are the conv zero padding), channels [C, Cp) are zero padding up to a multiple of 32.
 *  psnd_conv1d_cl:  Y[r][co] = sum_j sum_ci A_eff[r + off0 + j*dstep][ci] * W[j][co][ci]   (stride 1)
 *      forward       : W = pack [j][co][ci] of the weight, off0 = -pad, dstep = +dil
 *      backward-data : A = gY,  W = pack [j][ci][co],       off0 = +pad, dstep = -dil
 *    A_eff = A + A2 * (AM > 0 ? 1 : a2_slope): the gradient of a conv output that was handed out both raw (A)
 *            and through leaky_relu (A2, with AM the activated output) is combined while it is staged.
 *            a_eff_out (N, Lp, Ca) or NULL: A_eff written back (the gradient that continues along a residual branch).
 *    epilogue: v = acc (+ bias[co]); v *= (mask_src > 0 ? 1 : mask_slope) when mask_src; v += res when res;
 *              rows outside the clip -> 0; out_raw = v, out_act = leaky_relu(v, act_slope) (either may be NULL).
 *    replaces F.leaky_relu + Conv1d + bias (+ residual add)  (hifi_gan.py:56-62, 84-88) and their backward.
 *  psnd_conv1d_cl_wgrad: gw[j][co][ci] = sum_r g[r][co] * xa[r + off0 + j*dstep][ci] as S partial slabs over row
 *              ranges, gw_part fp32 [S][k][Cb][Ca] and gbias_part [S][Cb] (may be NULL), every element written (no
 *              zero fill, no atomics); S = psnd_conv1d_cl_wgrad_splits(N, Lp, Ca, Cb, k) (host helper).
 *              g_out = g materialised (may be NULL); g = G1 + G2*leaky'(GM).
 *  psnd_conv1d_prep: weight norm w = g*v/||v|| (norm over dim 0, as torch weight_norm) -> bf16 packs
 *              wf [k][Cb][Ca] and wb [k][Ca][Cb] (for k <= 3 both in MFMA B-fragment order: tap j, 32-column tile, 16-channel
 *              step, lane (c%16/8)*32 + n%32, 8 channels - an opaque layout shared by prep and conv), zero-padded bias (Cb).  psnd_conv1d_wnorm_bwd: adds the S
 *              slabs up and runs the weight-norm backward: (g_v, g_g) and gbias (Cb, may be NULL).
 *  psnd_to_cl / psnd_from_cl: (N,C,T) fp32 <-> CL bf16 (preop 1 = log1p on the way in). */
int psnd_conv1d_cl(const void *A, const void *A2, const void *AM, float a2_slope, const void *W, const float *bias,
                   const void *res, const void *mask_src, int64_t N, int Lp, int L, int HP, int Ca, int Cb, int k,
                   int off0, int dstep, float act_slope, float mask_slope, void *out_raw, void *out_act,
                   void *a_eff_out, void *stream);
int psnd_conv1d_cl_wgrad_splits(int64_t N, int Lp, int Ca, int Cb, int k);
/* Two chained convs (3, 7 or 11 taps each) of a residual pair in one launch (csrc/psnd_conv_pair.hip; hifi_gan.py:56-62 `leaky -> conv(d) -> leaky ->
 * conv(1) -> + x` and the input-gradient chain of the same pair):
 *      mid = leaky( (conv(A; W1, taps off1 + t*dstep1) + bias1) * (M1 > 0 ? 1 : m1_slope), act1_slope )   -> mid_out (may be NULL)
 *      out = (conv(mid; W2, taps off2 + t*dstep2) + bias2) * (M2 > 0 ? 1 : m2_slope) + res               -> out_raw, out_act
 * A, M1, M2, res, mid_out, out_*: CL bf16 (N, Lp, C); W1, W2: the [k][C][C] packs of psnd_conv1d_prep (forward: the [j][co][ci] pack,
 * input gradient: the [j][ci][co] pack with mirrored taps); bias / masks / res may be NULL; rows outside the clip are written as zero.
 * Same values as two psnd_conv1d_cl launches (mid is rounded to bf16 in both).  Covered: k = 3, C = 128 or 256, both tap reaches <= 8,
 * with or without masks (forward and input-gradient form); since round 5 also, WITHOUT masks (the forward order of a pair): k = 7 / 11 at
 * C = 32 / 64 / 128 / 256 and k = 3 at C = 32 / 64, first conv reach <= 25, second <= 8 (hifi_gan.py:32-63: kernel sizes 3 / 7 / 11,
 * dilations 1 / 3 / 5, then 1).  Ask psnd_conv1d_cl_pair_supported (1 / 0) first; PSND_E_UNSUPPORTED otherwise. */
int psnd_conv1d_cl_pair_supported(int C, int k, int off1, int dstep1, int off2, int dstep2);
int psnd_conv1d_cl_pair(const void *A, const void *W1, const float *bias1, const void *M1, float m1_slope, float act1_slope,
                        void *mid_out, const void *W2, const float *bias2, const void *M2, float m2_slope, const void *res,
                        int64_t N, int Lp, int L, int HP, int C, int k, int off1, int dstep1, int off2, int dstep2,
                        float act2_slope, void *out_raw, void *out_act, void *stream);
/* The weight gradients of n (<= 32) convs over the same N x Lp rows in one launch: per conv the operands and slabs of psnd_conv1d_cl_wgrad
 * with a plain gradient (g = the conv's combined output gradient (N, Lp, Cb), xa = its activated input (N, Lp, Ca), taps off0 + j * dstep;
 * gbias_part may be NULL) and `splits` row ranges = slabs.  psnd_conv1d_cl_wgrad_multi_splits(N, Lp, Ca, Cb, k, n): the number to use for n
 * convs of that shape; convs of another shape in the same launch (a model's head / tail) take the same number. */
typedef struct psnd_wgrad_desc {
    const void *g, *xa;
    float *gw_part, *gbias_part;
    int off0, dstep;
    int Ca, Cb, k, splits;
} psnd_wgrad_desc;
int psnd_conv1d_cl_wgrad_multi_splits(int64_t N, int Lp, int Ca, int Cb, int k, int n_convs);
int psnd_conv1d_cl_wgrad_multi(const psnd_wgrad_desc *d, int n, int64_t N, int Lp, void *stream);
/* A CHAIN of such pairs in one launch (csrc/psnd_conv_chain.hip; forward only: no masks): the pairs of a ResBlock1 (hifi_gan.py:56-62),
 * pair i + 1 reading the activated output and the residual stream of pair i on the chip.  Values bit-identical to n_pairs
 * psnd_conv1d_cl_pair launches; every pair's mid_out / out_raw / out_act (each may be NULL) is written as those launches would.  A, res: the
 * activated input and the residual stream of the first pair.  psnd_conv1d_cl_chain_rows(C, k, n_pairs, taps): rows a workgroup OWNS of the 64
 * it computes (the rest is recomputed by its neighbours), 0 = unsupported (taps: off1, dstep1, off2, dstep2 per pair; k = 3, C = 256,
 * reach <= 8, 1 ... 4 pairs, >= 16 rows left).  psnd_conv_chain_stats: out2 = { chain launches, pairs they carried }.
 * With M1 / M2 on every pair the launch is the INPUT-GRADIENT chain of those pairs walked backwards (the values of psnd_conv1d_cl_pair
 * with masks, transposed packs, mirrored taps): mid = conv(A; W1) * (M1 > 0 ? 1 : m1_slope), out = conv(mid; W2) * (M2 > 0 ? 1 : m2_slope)
 * + A; res == A, activation slopes 1, out_act NULL, out_raw of pair i is the input of pair i + 1. */
typedef struct psnd_chain_pair {
    const void *W1;
    const float *bias1;
    float act1_slope;
    void *mid_out;
    const void *W2;
    const float *bias2;
    int off1, dstep1, off2, dstep2;
    float act2_slope;
    void *out_raw, *out_act;
    const void *M1, *M2;        /* the input-gradient form (below): leaky' masks of the two convs' outputs, or both NULL */
    float m1_slope, m2_slope;
} psnd_chain_pair;
int psnd_conv1d_cl_chain_rows(int C, int k, int n_pairs, const int *taps);
/* the rows a workgroup owns for a launch over R = N * Lp rows and its row tile (*mr_out: 1 = 32 computed rows, 2 = 64; may be NULL):
 * 64-row tiles (32-row tiles exist for A/B runs, PSND_CHAIN_MR=1); 0 = unsupported */
int psnd_conv1d_cl_chain_plan(int C, int k, int n_pairs, const int *taps, int64_t R, int *mr_out);
int psnd_conv1d_cl_chain(const void *A, const void *res, const psnd_chain_pair *pairs, int n_pairs, int64_t N, int Lp, int L, int HP,
                         int C, int k, void *stream);
void psnd_conv_chain_stats(long long *out2);
/* host-side launch counters of the conv kernels' tile instances: out4 = { forward / input-gradient launches with 64-row
 * workgroup tiles, with 128-row tiles, paired backward launches with 64-row tiles, with 128-row tiles } (out4 may be NULL);
 * reset != 0 clears them.  Test instrumentation: lets a parity test assert that its shape ran the instance it covers. */
/* ---- the same passes with the magnitude side BIN-FASTEST, (N, F, K) (psnd_stft_mag_nfk): (N, F, K) is the channels-last order (frame t
 *      of clip n = row n*Lp + HP + t, bin c = channel c), so the layout changes around the conv stack become plain streams, no transposes.
 *  psnd_to_cl_nfk            : x_nfk (N,F,K) fp32 -> CL bf16 (N,Lp,Cp), preop 1 = log1p; halo rows / padded channels written as zeros
 *  psnd_mask_head_l1_fwd_nfk : est_nfk = sigmoid(y) * mag_nfk; ref_nfk + part (both or neither): part[b] = sum |est - ref| of workgroup b
 *                              (psnd_mask_head_l1_blocks_nfk doubles)
 *  psnd_mask_head_l1_bwd_nfk : gy (CL) = (gest_nfk (may be NULL) + coef * g[0] * sign(est - ref)) * mag * s (1 - s)
 *  psnd_mel_fwd_nfk / psnd_mel_l1_fwd_nfk : psnd_mel_fwd / psnd_mel_l1_fwd reading mag_nfk (N,F,K); outputs stay (N,M,F)
 *  psnd_mel_bwd_nfk / psnd_mel_l1_bwd_nfk : psnd_mel_bwd / psnd_mel_l1_bwd writing gmag_nfk (N,F,K)
 *  Cp % 8 == 0, Cp >= round_up(K, 8); N*F*K*4 < 2^32 bytes. */
int psnd_to_cl_nfk(const float *x_nfk, int64_t N, int K, int64_t F, int Lp, int HP, int Cp, int preop, void *out, void *stream);
int64_t psnd_mask_head_l1_blocks_nfk(int64_t N, int64_t F, int K);
int psnd_mask_head_l1_fwd_nfk(const void *y, const float *mag_nfk, const float *ref_nfk, int64_t N, int K, int64_t F, int Lp, int HP, int Cp,
                              float *est_nfk, double *part, void *stream);
int psnd_mask_head_l1_bwd_nfk(const float *gest_nfk, const float *mag_nfk, const void *y, const float *est_nfk, const float *ref_nfk,
                              const float *g, float coef, int64_t N, int K, int64_t F, int Lp, int HP, int Cp, void *gy, void *stream);
int psnd_mel_fwd_nfk(const float *mag_nfk, int64_t N, int64_t F, int M, int K, const void *mel_plan, int log_kind, float log_offset,
                     float pre_clamp_min, float clamp_lo, float clamp_hi, float *out, float *mel_lin, void *stream);
int psnd_mel_bwd_nfk(const float *gout, const float *mel_lin, int64_t N, int64_t F, int M, int K, const void *mel_plan, int log_kind,
                     float log_offset, float pre_clamp_min, float clamp_lo, float clamp_hi, float *gmag_nfk, void *stream);
int psnd_mel_l1_fwd_nfk(const float *mag_nfk, int64_t N, int64_t F, int M, int K, const void *mel_plan, int log_kind, float log_offset,
                        float pre_clamp_min, float clamp_lo, float clamp_hi, const float *ref, float *mel_lin, double *part, void *stream);
int psnd_mel_l1_bwd_nfk(const float *ref, const float *mel_lin, const float *g, float coef, int64_t N, int64_t F, int M, int K,
                        const void *mel_plan, int log_kind, float log_offset, float pre_clamp_min, float clamp_lo, float clamp_hi,
                        float *gmag_nfk, void *stream);
/* ---- a spectral-masking recipe's loss without its intermediate tensors (round 3):
 *      w1 * F.l1_loss(est, mag_ref) + w2 * F.l1_loss(log_mel(est), mel_ref),  est = sigmoid(from_cl(y)) * mag
 *  psnd_mask_head_l1_fwd : psnd_mask_head_fwd + part[b] = sum |est - ref| of workgroup b (psnd_mask_head_l1_blocks doubles)
 *  psnd_mel_l1_fwd       : psnd_mel_fwd that writes only the linear mel + part[w] = sum |log_mel - ref| of wave w (psnd_mel_l1_blocks)
 *  psnd_l1_loss_combine  : out[0] = sum_i scale[i] * sum(parts[i]), scale = weight / numel (host arrays of <= 4 device pointers);
 *                          nan_flag (may be NULL): nan_flag[0] = 1 if that loss is NaN, else 0 (the trainer's `loss != loss`, trainer.py:205)
 *  psnd_mel_l1_bwd       : gmag = W^T (coef * g[0] * sign(log_mel - ref) * dlog) with the sign formed on operand load (g: device scalar)
 *  psnd_mask_head_l1_bwd : psnd_mask_head_bwd on gest (may be NULL) + coef * g[0] * sign(est - ref)                              */
int64_t psnd_mask_head_l1_blocks(int64_t N, int64_t T, int Cp);
int psnd_mask_head_l1_fwd(const void *y, const float *mag, const float *ref, int64_t N, int C, int64_t T, int Lp, int HP, int Cp,
                          float *est, double *part, void *stream);
int psnd_mask_head_l1_bwd(const float *gest, const float *mag, const void *y, const float *est, const float *ref, const float *g,
                          float coef, int64_t N, int C, int64_t T, int Lp, int HP, int Cp, void *gy, void *stream);
int64_t psnd_mel_l1_blocks(int64_t N, int64_t F, int M);
int psnd_mel_l1_fwd(const float *mag, int64_t N, int64_t F, int M, int K, const void *mel_plan, int log_kind, float log_offset,
                    float pre_clamp_min, float clamp_lo, float clamp_hi, const float *ref, float *mel_lin, double *part, void *stream);
int psnd_mel_l1_bwd(const float *ref, const float *mel_lin, const float *g, float coef, int64_t N, int64_t F, int M, int K,
                    const void *mel_plan, int log_kind, float log_offset, float pre_clamp_min, float clamp_lo, float clamp_hi,
                    float *gmag, void *stream);
/* flag[0] = 1.0 if any of x[0 .. n) is NaN, else 0.0 - the device-side form of the trainer's `loss != loss` (trainer.py:205) */
int psnd_nan_flag(const float *x, int64_t n, float *flag, void *stream);
int psnd_l1_loss_combine(const double *const *parts, const int64_t *nb, const double *scale, int terms, float *out, float *nan_flag, void *stream);
int psnd_conv_stats(int64_t *out4, int reset);
/* the same for the residual-pair launches: out4 = { psnd_conv1d_cl_pair launches with 32-row tiles, with 64-row tiles,
 * psnd_conv1d_cl_pair_bwd launches that carried a pair, weight-gradient row ranges of the last psnd_conv1d_cl_pair_bwd launch }. */
int psnd_conv_pair_stats(int64_t *out4, int reset);
int psnd_conv1d_cl_wgrad(const void *G1, const void *G2, const void *GM, float g2_slope, const void *xa, int64_t N,
                         int Lp, int Ca, int Cb, int k, int off0, int dstep, float *gw_part, float *gbias_part,
                         void *g_out, void *stream);
int psnd_conv1d_prep(const float *v, const float *g, const float *bias, int Cout, int Cin, int k, int Cb, int Ca,
                     void *wf, void *wb, float *bias_padded, void *stream);
/* ---- ConvTranspose1d(Cin, Cout, K = 2 * stride, stride, padding <= stride) of the HiFi-GAN upsamplers (hifi_gan.py:109,
 *  118-121) in polyphase form on the CL kernels:  y[t] = x[i] w[:, :, phi] + x[i-1] w[:, :, phi + stride],  t + padding =
 *  i * stride + phi.  Low-resolution CL buffer (N, Lp, Cip) with clip rows [HP, HP + L), HP >= 1; high-resolution CL buffer
 *  (N, LpO, Cr) with clip rows [HPO, HPO + L * stride), HPO >= padding and stride - padding rows behind the clip; rows outside
 *  the clip of every output are written as zeros or left untouched (allocate the outputs zeroed).
 *  psnd_convtr1d_prep : weight norm over dim 0 of v (Cin, Cout, K) (per INPUT channel, as torch weight_norm does for
 *                       nn.ConvTranspose1d) -> bf16 packs wf, wb (2 * stride * Cr * Cip elements each, opaque fragment order) and
 *                       bias_rep (stride * Cr floats: the bias once per phase).
 *  psnd_convtr1d_cl_fwd: out_raw = y, out_act = leaky_relu(y, act_slope) (either may be NULL).
 *  psnd_convtr1d_cl_bwd: g = g_raw + g_act * leaky'(act) (either part may be NULL) -> gx (N, Lp, Cip), g_eff (N, LpO, Cr; the
 *                       combined gradient, required when g_act is given: its column sums are the bias gradient) and the
 *                       weight-gradient slabs gw_part fp32 [S][2][Cip][stride * Cr], S = psnd_convtr1d_cl_wgrad_splits(...).
 *                       gw_part == NULL: the input-gradient launch alone; gx == NULL: the weight-gradient launch alone (g_eff as
 *                       the first call wrote it) - the two roles of one backward on two streams.
 *  psnd_convtr1d_wnorm_bwd: slabs -> g_v (Cin, Cout, K), g_g (Cin). */
int psnd_convtr1d_prep(const float *v, const float *g, const float *bias, int Cin, int Cout, int K, int stride, int Cr, int Cip,
                       void *wf, void *wb, float *bias_rep, void *stream);
/* psnd_convtr1d_prep for n transposed convs in ONE launch.  descs_dev: device array of n records
 *   { const float *v, *g, *bias; void *wf, *wb; float *bp; int Cin, Cout, K, u, Cr, Cip, blk0, pad; }   (80 bytes; blk0 = sum of the Cin of the
 *   records before it), total_blocks = the sum of all Cin.  Same packs as psnd_convtr1d_prep; the pads of wf / wb are not written (zero once). */
int psnd_convtr1d_prep_multi(const void *descs_dev, int n, int total_blocks, void *stream);
int psnd_convtr1d_cl_fwd(const void *xa, const void *wf, const float *bias_rep, int64_t N, int Lp, int L, int HP, int Cip, int Cr,
                         int stride, int padding, int LpO, int HPO, float act_slope, void *out_raw, void *out_act, void *stream);
int psnd_convtr1d_cl_wgrad_splits(int64_t N, int Lp, int Cip, int Cr, int stride);
int psnd_convtr1d_cl_bwd(const void *g_raw, const void *g_act, const void *act, float act_slope, const void *wb, const void *xa,
                         int64_t N, int Lp, int L, int HP, int Cip, int Cr, int stride, int padding, int LpO, int HPO, void *gx,
                         void *g_eff, float *gw_part, void *stream);
int psnd_convtr1d_wnorm_bwd(const float *gw_part, int splits, const float *v, const float *g, int Cin, int Cout, int K, int stride,
                            int Cr, int Cip, float *gv, float *gg, void *stream);
/* out = leaky_relu((a + b + c + d) / count, slope) over `count` (1..4) bf16 buffers of n elements (n % 8 == 0): the mean of a
 * stage's resblocks and the activation in front of the next upsampler (hifi_gan.py:122-131); backward gin = g * leaky'(y) / count. */
int psnd_cl_mean_act_fwd(const void *a, const void *b, const void *c, const void *d, int count, float slope, void *out, int64_t n,
                         void *stream);
int psnd_cl_mean_act_bwd(const void *g, const void *y, int count, float slope, void *gin, int64_t n, void *stream);
/* out_a = a[0] + .. + a[na-1], out_b = b[0] + .. + b[nb-1] over bf16 buffers of n elements (n % 8 == 0; fp32 accumulation, one rounding), both in ONE
 * launch: the gradients arriving at an upsampler's raw / activated outputs from the resblocks of its stage (hifi_gan.py:122-131).  a, b: HOST
 * arrays of na, nb (0..4) device pointers. */
int psnd_cl_sum2(const void *const *a, int na, void *out_a, const void *const *b, int nb, void *out_b, int64_t n, void *stream);
/* out[c] = sum over the rows of a channels-last bf16 matrix g (rows, C) in fp32, C % 8 == 0, 8 <= C <= 256: the bias gradient of a transposed
 * conv (reference hifi_gan.py:107-110; replaces a library column reduction).  part: fp32 scratch of psnd_cl_colsum_splits(rows, C) * C
 * elements; two launches, fixed summation order.  Lp > 0: g is rows / Lp clip buffers of Lp rows and only the rows [lo, hi) of each are
 * summed (the others are never read: they may be unwritten); Lp = 0: every row. */
int psnd_cl_colsum_splits(int64_t rows, int C);
int psnd_cl_colsum(const void *g, int64_t rows, int C, int Lp, int lo, int hi, float *part, float *out, void *stream);
/* psnd_conv1d_prep for n convs in ONE launch (one workgroup per 8 output channels: every store a 16-byte piece of the packs).
 * descs_dev: device array of n records
 *   { const float *v, *g, *bias; void *wf, *wb; float *bp; int Cout, Cin, k, Cb, Ca, blk0; }   (72 bytes, blk0 = sum of
 *   ceil(Cout / 8) of the records before it), total_blocks = that sum over all records, max_row = the largest Cin * k
 *   (<= 10240: the 8 rows of a workgroup live in LDS; larger layers take psnd_conv1d_prep).  Same packs, bit for bit, as
 *   psnd_conv1d_prep.  which: 1 = forward pack + bias, 2 = backward pack, 3 = both (the backward pack can be written when the backward
 *   starts: lines written by 16-byte stores are read fastest while they are fresh).  The pad regions of wf / wb / bp beyond the 8-channel
 *   groups are not written (zero them once). */
int psnd_conv1d_prep_multi(const void *descs_dev, int n, int total_blocks, int max_row, int which, void *stream);
/* psnd_conv1d_wnorm_bwd for up to PSND_WNORM_MAX convs (the six of a ResBlock1, the 26 of the separator body) in one launch; descs is a HOST array,
 * passed to the kernel by value (nothing is uploaded, the launch can be captured in a hipGraph).  A launch whose rows all have Cin k < 2048 and
 * at most 16 slabs runs 256 threads; there a conv with Cin and Ca multiples of 4 takes one workgroup per EIGHT output channels (every load in
 * flight before the first wait, v read once), any other conv of the launch one workgroup per channel.  The sums are grouped as in the
 * one-channel form: the same bits either way, as from psnd_conv1d_wnorm_bwd. */
#define PSND_WNORM_MAX 32
typedef struct psnd_wnorm_desc {
    const float *gw_part, *gbias_part;      /* slabs of psnd_conv1d_cl_wgrad / psnd_conv1d_cl_bwd (gbias_part may be NULL) */
    const float *v, *g;                     /* weight_v (Cout,Cin,k), weight_g (Cout)                                      */
    float *gv, *gg, *gbias;                 /* outputs (gbias may be NULL)                                                 */
    int splits, Cout, Cin, k, Cb, Ca;
} psnd_wnorm_desc;
int psnd_conv1d_wnorm_bwd_multi(const psnd_wnorm_desc *descs, int n, void *stream);
/* backward of one conv in ONE launch: gx = input gradient (Ca channels, via the transposed pack wb, taps mirrored) and the
 * partial weight-gradient slabs gw_part / gbias_part (as psnd_conv1d_cl_wgrad), both from g = G1 + G2 * leaky'(GM); g_out (may
 * be NULL) receives the combined g for the residual branch (needs G2).  gx_mask / gx_res (CL bf16, Ca channels, may be NULL):
 * epilogue of the input gradient, gx = gx * leaky'(gx_mask; gx_mask_slope) + gx_res - i.e. the NEXT conv's combined incoming gradient
 * (its own leaky-relu derivative and the residual branch) is formed here, so that conv's backward needs no combine on load.
 * gw_part == NULL: the input gradient alone (the weight gradient is left to psnd_conv1d_cl_wgrad_multi). */
int psnd_conv1d_cl_bwd(const void *G1, const void *G2, const void *GM, float g2_slope, const void *wb, const void *xa,
                       int64_t N, int Lp, int L, int HP, int Ca, int Cb, int k, int pad, int dil, void *gx, void *g_out,
                       const void *gx_mask, float gx_mask_slope, const void *gx_res, float *gw_part, float *gbias_part,
                       void *stream);
/* Backward of a whole residual pair (`leaky -> conv1(d) -> leaky -> conv2(1) -> + x`, hifi_gan.py:56-62) as ONE launch: the input gradients
 * of both convs chained on chip (psnd_conv1d_cl_pair's body with the transposed packs wb2 / wb1, mirrored taps, the leaky' masks M1 = the
 * activated conv1 output and M2 = the activated pair input, res = G the gradient on the residual stream: g_mid = gradient wrt conv1's
 * output, gx = gradient wrt the pair's input), the weight-gradient slabs of conv2 (gradient G, input xa_a = M1; gw_a / gb_a) and the slabs
 * of ANOTHER conv whose gradient an earlier launch produced (G_b, xa_b with taps off_b + t * dstep_b; gw_b / gb_b; all NULL: none) -
 * in a chain walked backwards that is conv1 of the pair handled before.  G == NULL: only the `_b` weight gradient (the chain's last
 * conv1).  Slabs: psnd_conv1d_cl_pair_bwd_splits(N, Lp, C, k) per conv, layout as psnd_conv1d_cl_wgrad.  C = 256, k = 3 and
 * psnd_conv1d_cl_pair_bwd_supported(...) == 1, PSND_E_UNSUPPORTED otherwise. */
int psnd_conv1d_cl_pair_bwd_supported(int C, int k, int pad2, int dil2, int pad1, int dil1);
int psnd_conv1d_cl_pair_bwd_splits(int64_t N, int Lp, int C, int k);
int psnd_conv1d_cl_pair_bwd(const void *G, const void *wb2, const void *M1, float m1_slope, void *g_mid, const void *wb1, const void *M2,
                            float m2_slope, const void *res, int64_t N, int Lp, int L, int HP, int C, int k, int pad2, int dil2,
                            int pad1, int dil1, void *gx, const void *xa_a, float *gw_a, float *gb_a, const void *G_b,
                            const void *xa_b, int off_b, int dstep_b, float *gw_b, float *gb_b, void *stream);
int psnd_conv1d_wnorm_bwd(const float *gw_part, const float *gbias_part, int splits, const float *v, const float *g,
                          int Cout, int Cin, int k, int Cb, int Ca, float *gv, float *gg, float *gbias, void *stream);
int psnd_to_cl(const float *x, int64_t N, int C, int64_t T, int Lp, int HP, int Cp, int preop, void *out, void *stream);
/* out = tanh(from_cl(x)) - the generator's output non-linearity (vocoders/hifi_gan.py:134-135) inside the layout change - and its backward
 * gx = to_cl(g * (1 - out_fwd^2)) (halo rows / padded channels written as zeros). */
int psnd_from_cl_tanh(const void *x, int64_t N, int C, int64_t T, int Lp, int HP, int Cp, float *out, void *stream);
int psnd_to_cl_tanh_bwd(const float *g, const float *out_fwd, int64_t N, int C, int64_t T, int Lp, int HP, int Cp, void *gx, void *stream);
int psnd_from_cl(const void *x, int64_t N, int C, int64_t T, int Lp, int HP, int Cp, float *out, void *stream);
/* mask head of a spectrogram-masking model: est (N,C,T) fp32 = sigmoid(from_cl(y)) * mag in one pass; backward
 * gy (CL bf16) = to_cl(gest * mag * s (1 - s)), s = sigmoid(y) recomputed (halo rows / padded channels written as zeros). */
int psnd_mask_head_fwd(const void *y, const float *mag, int64_t N, int C, int64_t T, int Lp, int HP, int Cp, float *est,
                       void *stream);
int psnd_mask_head_bwd(const float *gest, const float *mag, const void *y, int64_t N, int C, int64_t T, int Lp, int HP, int Cp,
                       void *gy, void *stream);

/* ---- dense contractions of models/modules.py on the matrix cores, exact fp32 (v_mfma_f32_32x32x2_f32) --------------------
 * psnd_linear1x1_fwd: y[n][co][t] = sum_ci w[co][ci] x[n][ci][t] + bias[co] (, relu) - the 1x1 Conv1d projections
 *   (modules.py:21-22 linear_kvq / linear, :93-95 the feed-forward pair).  x (N,Cin,T), w (Cout,Cin), y (N,Cout,T) fp32.
 *   bf16 != 0: both operands are rounded to bf16 while they are staged (v_mfma_f32_32x32x16_bf16, fp32 accumulate, 16x the matrix
 *   rate) - what the modules select under torch.autocast(bfloat16); 0: exact fp32 products.
 * psnd_linear1x1_bwd: gy' = gy where ymask > 0 (ymask = the relu output y, or NULL); gx = w^T gy' (NULL: skipped),
 *   gw = sum_{n,t} gy' x^T via S = psnd_linear1x1_wgrad_slabs(...) partial slabs gw_part (S*Cout*Cin floats), gbias = sum gy'.
 * psnd_mha_fwd: MultiHeadAttention.scale_dot_att over all heads (modules.py:38-48, 61-79).  kvq (N, 3C, T): rows [0,C) keys,
 *   [C,2C) values, [2C,3C) queries (the reference's chunk order), head h = channels [h*d, (h+1)*d), d = C/H <= 64 (PSND_E_UNSUPPORTED
 *   otherwise), batch index b = h*N + n.  mask (N,T) bytes, 1 = padding, or NULL: padded keys get no
 *   weight, padded queries are zeroed.  out (N, C, T) (heads unfolded); att (H*N, T_key, T_query) or NULL - the scores never
 *   leave the chip otherwise; stats (H*N, T, 2): per query column (max, 1/sum), kept for the backward.
 *   bf16 != 0: the operands of the four score / accumulate products (K, Q, V and the probabilities) are rounded to bf16 on their
 *   way to the matrix cores; scores, softmax statistics and accumulation stay fp32 (selected under torch.autocast(bfloat16)).
 *   bf16 == 2 (round 6; att == NULL only): as 1, and kvq is read and out WRITTEN as bf16 tensors (2-byte elements, same shapes - what
 *   psnd_linear1x1_fwd_ex writes with io_h = 2 and takes with io_h = 1): the values multiplied are the same, the kernels convert
 *   nothing in their loops.
 * psnd_mha_bwd: gkvq (N, 3C, T) from gout (N, C, T) and, optionally, gatt (needs att).  delta (H*N, T) scratch.  bf16 as above (the
 *   probabilities are recomputed from the saved statistics: pass the forward's choice); bf16 == 2 (att, gatt NULL): kvq, out and gout
 *   are read and gkvq WRITTEN as bf16 (psnd_linear1x1_bwd_ex writes gout with io_h = 2 and takes gkvq with io_h = 1); stats, delta fp32
 *   (delta is then formed by the query-gradient kernel from the fragments it holds - no separate pass over out and gout; psnd_mha_bwd_parts
 *   takes bf16 = 2 with parts = 7 only). */
int psnd_linear1x1_fwd(const float *x, const float *w, const float *bias, int64_t N, int Cin, int Cout, int64_t T, int relu, int bf16,
                       float *y, void *stream);
int64_t psnd_linear1x1_wgrad_slabs(int64_t N, int Cin, int Cout, int64_t T);
int psnd_linear1x1_bwd(const float *gy, const float *ymask, const float *x, const float *w, int64_t N, int Cin, int Cout, int64_t T,
                       int bf16, float *gx, float *gw, float *gw_part, float *gbias, void *stream);
/* psnd_linear1x1_bwd with gx = w^T gy' + gx_addend (N, Cin, T; NULL: none): the gradient that reaches x along a residual connection
 * (`x + self.drop_out(...)` before the GroupNorm, modules.py:56-58, 114-116) is added in the GEMM's epilogue - autograd's separate
 * accumulation pass over both tensors disappears. */
int psnd_linear1x1_bwd_acc(const float *gy, const float *ymask, const float *x, const float *w, int64_t N, int Cin, int Cout, int64_t T,
                           int bf16, const float *gx_addend, float *gx, float *gw, float *gw_part, float *gbias, void *stream);
/* ... or with gx = (gx_mask > 0) ? w^T gy' : 0, gx_mask (N, Cin, T; NULL: none; not together with gx_addend): x is the output of a ReLU
 * (Conv1d -> ReLU -> Conv1d, modules.py:93-95; gx_mask = x) and gx is wanted for the ReLU's input.  The layer before the ReLU then calls
 * with ymask = NULL: its two GEMMs and its bias sum read the gradient alone instead of gradient + mask.
 * io_h (with bf16 != 0; 0: every tensor is fp32): 1 = gy is STORED as bf16 (2-byte elements, same shape; ymask NULL), 2 = x, gx_mask and gx
 * are (gx_addend NULL) - the hidden tensor of that pair under torch.autocast(bfloat16): the products round their operands to bf16 when
 * they load them, so the values multiplied are the same and the tensor and its gradient move at half the bytes.  The weight, bias and
 * parameter gradients are always fp32. */
int psnd_linear1x1_bwd_ex(const void *gy, const float *ymask, const void *x, const float *w, int64_t N, int Cin, int Cout, int64_t T, int bf16,
                          int io_h, int64_t ld_h, const float *gx_addend, const void *gx_mask, void *gx, float *gw, float *gw_part, float *gbias,
                          void *stream);
/* psnd_linear1x1_fwd with io_h (bf16 != 0): 1 = x is stored as bf16, 2 = y is (see psnd_linear1x1_bwd_ex); 0 = psnd_linear1x1_fwd.
 * ld_h (both entry points): row pitch in elements of the bf16-stored tensors - (N, C, ld_h) in memory, the first T frames of a row used;
 * 0 = T.  They are the caller's own tensors between two calls: rows that start on 128-byte lines (ld_h a multiple of 64) spare the
 * GEMMs the straddling loads and stores of odd row lengths. */
int psnd_linear1x1_fwd_ex(const void *x, const float *w, const float *bias, int64_t N, int Cin, int Cout, int64_t T, int relu, int bf16, int io_h,
                          int64_t ld_h, void *y, void *stream);
int psnd_mha_fwd(const float *kvq, const unsigned char *mask, int64_t N, int H, int C, int64_t T, float *out, float *att, float *stats,
                 int bf16, void *stream);
int psnd_mha_bwd(const float *kvq, const unsigned char *mask, const float *out, const float *att, const float *stats, const float *gout,
                 const float *gatt, int64_t N, int H, int C, int64_t T, float *delta, float *gkvq, int bf16, void *stream);
/* psnd_mha_bwd in parts (bit mask): 1 = delta, 2 = key / value gradients, 4 = query gradients (7 = psnd_mha_bwd).  The two gradient
 * kernels need `delta` only and write disjoint rows of gkvq: a caller may enqueue them on two streams behind the delta launch. */
int psnd_mha_bwd_parts(const float *kvq, const unsigned char *mask, const float *out, const float *att, const float *stats, const float *gout,
                       const float *gatt, int64_t N, int H, int C, int64_t T, float *delta, float *gkvq, int bf16, int parts, void *stream);

/* ---- transformer blocks of models/modules.py: the parts that are not plain GEMMs --------------------------
 *  psnd_groupnorm1_fwd: y = GroupNorm(1, C)(x + res) [relu]  (modules.py:30,58 / :98,114-116): mean / variance over
 *      (C x T) per sample (accumulated in double), per-channel affine.  x, res (may be NULL), y : (N,C,T) fp32;
 *      stats : (N,2) {mean, rstd} saved for backward; ws : (N,C,2) double scratch (caller owned, overwritten;
 *      PSND_GN_WS_DOUBLES(C) doubles per sample): one pair of sums per row, written and then added up in a fixed order - no
 *      atomics, the statistics are the same bits from run to run (round 6; rounds 3-5 took 32 doubles per sample).
 *  psnd_groupnorm1_bwd: gx (gradient wrt x and wrt res), ggamma, gbeta (C) - all fully overwritten; ws as above.
 *  psnd_groupnorm1_drop_fwd / _drop_bwd: the same with dropout in front of the sum, y = GroupNorm(1, C)(x * keep * scale + res) [relu]
 *      (modules.py:54-58, :112-116), the mask never in memory: element i of the contiguous (N,C,T) x is kept iff word i % 4 of
 *      Philox4x32-10(counter = {q lo, q hi, call lo, call hi} with q = i / 4, key = {seed lo, seed hi}) is >= thr; key : the {seed, call}
 *      pair of this application in DEVICE memory (psnd_rng_next wrote it; the same pair for forward and backward), thr =
 *      min(2^32 - 1, floor(p * 2^32)), scale = 1 / (1 - p).  A dropped element contributes exactly res.  _drop_bwd: gres = the gradient of
 *      the sum (written when gres is not NULL: needs res and a buffer of its own), gx = gres * keep * scale (an exact zero where dropped).
 *  psnd_rng_seed: state : two uint64 {seed, call} in device memory, overwritten by a one-thread kernel on the stream.
 *  psnd_rng_next: key_out = state, then state.call += 1 - one thread, stream ordered and capturable: every replay of a hipGraph that holds
 *      the launch advances the state, so every step draws fresh masks.
 *  psnd_softmax_keys_fwd: in place on scores (B,Tk,Tq): a = softmax over Tk of scale*s with key-padded rows at -inf,
 *      query-padded columns set to 0 (modules.py:66-76); mask (B,T) uint8, 1 = padded, or NULL.
 *  psnd_softmax_keys_bwd: gscores = scale * a * (gatt - sum_tk gatt*a). */
#define PSND_GN_WS_DOUBLES(C) (2 * (size_t)(C))
/* PositionalEncoding.forward (modules.py:119-145): y = x * scale + pe[:, :T] in one pass; x, y (N,C,T) fp32, pe (C, pe_len) rows (the module's
 * buffer (1, C, max_len)), pe_len >= T.  pe == NULL: y = x * scale (the backward: gx = g * scale). */
int psnd_posenc(const float *x, const float *pe, float scale, int64_t N, int C, int64_t T, int64_t pe_len, float *y, void *stream);
int psnd_groupnorm1_fwd(const float *x, const float *res, const float *gamma, const float *beta, int64_t N, int C,
                        int64_t T, float eps, int relu, float *y, float *stats, double *ws, void *stream);
int psnd_groupnorm1_bwd(const float *gy, const float *x, const float *res, const float *gamma, const float *y,
                        const float *stats, int64_t N, int C, int64_t T, int relu, float *gx, float *ggamma,
                        float *gbeta, double *ws, void *stream);
int psnd_groupnorm1_drop_fwd(const float *x, const float *res, const float *gamma, const float *beta, int64_t N, int C,
                             int64_t T, float eps, int relu, float *y, float *stats, double *ws, const uint64_t *key,
                             uint32_t thr, float scale, void *stream);
int psnd_groupnorm1_drop_bwd(const float *gy, const float *x, const float *res, const float *gamma, const float *y,
                             const float *stats, int64_t N, int C, int64_t T, int relu, float *gx, float *gres, float *ggamma,
                             float *gbeta, double *ws, const uint64_t *key, uint32_t thr, float scale, void *stream);
int psnd_rng_seed(uint64_t *state, uint64_t seed, uint64_t call, void *stream);
int psnd_rng_next(uint64_t *state, uint64_t *key_out, void *stream);
int psnd_softmax_keys_fwd(float *scores, const uint8_t *mask, int64_t B, int64_t T, float scale, void *stream);
int psnd_softmax_keys_bwd(const float *att, const float *gatt, int64_t B, int64_t T, float scale, float *gscores,
                          void *stream);

/* ---- models/sound.py: PreEmphasis (:66-81) and the reductions of multi_stft_loss (:106-133) -----------------
 *  psnd_preemphasis_fwd: y[n][t] = x[n][t] - coef * x[n][t-1] with x[n][-1] := x[n][1] (one reflect-padded sample,
 *      conv1d with the flipped filter [-coef, 1]);  x, y : (N, T) fp32 (the module's (N,1,T) is the same memory).
 *  psnd_preemphasis_bwd: the adjoint, gx fully overwritten.
 *  multi_stft_loss on magnitudes p, t : (N, K, F) fp32 per resolution (KF = K*F elements per clip):
 *  psnd_stft_loss_blocks(KF): workgroups per clip B of the partial pass (host helper).
 *  psnd_stft_loss_partial: part[(n*B + b)*3 + {0,1,2}] = sum (t-p)^2, sum t^2, sum |log(t+eps) - log(p+eps)| over
 *      chunk b of clip n (double; every entry written, no atomics).
 *  psnd_stft_loss_final: combines L <= 8 resolutions (host arrays parts[L] of device pointers, KF[L]) into
 *      out3 = {loss, sc_loss, mag_loss} (sound.py:119-133) and norms[(i*N + n)*2 + {0,1}] = ||t-p||_F, ||t||_F.
 *  psnd_stft_loss_bwd: one resolution; norms = that resolution's N pairs; g3 = DEVICE pointer to the upstream gradient
 *      of (loss, sc_loss, mag_loss); gp / gt (either may be NULL) = gradient wrt p / t, fully overwritten. */
int psnd_preemphasis_fwd(const float *x, int64_t N, int64_t T, float coef, float *y, void *stream);
int psnd_preemphasis_bwd(const float *gy, int64_t N, int64_t T, float coef, float *gx, void *stream);
int64_t psnd_stft_loss_blocks(int64_t KF);
int psnd_stft_loss_partial(const float *p_mag, const float *t_mag, int64_t N, int64_t KF, float eps, double *part,
                           void *stream);
int psnd_stft_loss_final(const double *const *parts, const int64_t *KF, int L, int64_t N, float *norms, float *out3,
                         void *stream);
int psnd_stft_loss_bwd(const float *p_mag, const float *t_mag, int64_t N, int64_t KF, float eps, const float *norms,
                       const float *g3, int L, float *gp, float *gt, void *stream);
/*  psnd_stft_bwd_msl: psnd_stft_loss_bwd (gp only) FUSED into psnd_stft_bwd for one resolution - the gradient of multi_stft_loss
 *      w.r.t. the predicted waveform in one launch: the adjoint recomputes |X| of `wav` (the prediction), forms
 *      d loss / d |X| = k1 (|X| - t) + c_mag sign(|X| - t) / (|X| + eps) from it and the target magnitudes t_mag (N, K, F) in
 *      registers (the magnitude gradient never exists in HBM) and continues as psnd_stft_bwd.  norms / g3 / L / eps as
 *      psnd_stft_loss_bwd; gwav (N, T) fully overwritten, or - accumulate != 0 - added to (the sum over the resolutions
 *      without separate add launches).  psnd_stft_bwd_msl_supported(n_fft, hop): 1 where the span-staged
 *      adjoint runs (n_fft 512 / 1024 / 2048, even hop up to n/2 resp. 256), else callers use the two-launch path. */
/*  psnd_stft_fwd_msl: psnd_stft_fwd (magnitude, centre framing) + psnd_stft_loss_partial FUSED for the prediction of one resolution:
 *      |X| is compared with t_mag (N, K, F) in registers and only the three sums leave the kernel - part[(n*B + b)*3 + {0,1,2}],
 *      B = psnd_stft_fwd_msl_blocks(T, n_fft, hop) entries per clip (0: this (n_fft, hop) is not covered - span-staged kernel,
 *      n_fft 512 / 1024 / 2048, one tile per workgroup).  psnd_stft_loss_final_blocks: psnd_stft_loss_final with the entries per
 *      clip given per resolution (blocks[L], host array; NULL = psnd_stft_loss_blocks(KF[i])). */
int64_t psnd_stft_fwd_msl_blocks(int64_t T, int n_fft, int hop);
int psnd_stft_fwd_msl(const float *wav, int64_t N, int64_t T, int n_fft, int hop, const void *plan, float mag_eps,
                      const float *t_mag, float eps, double *part, void *stream);
int psnd_stft_loss_final_blocks(const double *const *parts, const int64_t *KF, const int64_t *blocks, int L, int64_t N,
                                float *norms, float *out3, void *stream);
int psnd_stft_bwd_msl_supported(int n_fft, int hop);
int psnd_stft_bwd_msl(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing, const void *plan,
                      float mag_eps, const float *t_mag, const float *norms, const float *g3, int L, float eps,
                      int accumulate, float *gwav, void *stream);

/* ---- models/sound.py: InversePreEmphasis (:84-99) and VolNormConv (:7-60) ----------------------------------------------------------
 *  psnd_ipreemph_fwd: y[n][t] = tanh(w_ih x[n][t] + w_hh y[n][t-1]), y[n][-1] = 0 - the one-unit bias-free tanh RNN.  x, y : (N, T) fp32.
 *      w_ih, w_hh : DEVICE pointers to one float each (the RNN's own parameters: read at run time, so nothing the caller cached can go
 *      stale).  `warm` selects the instance:
 *        a multiple of 32 in [32, PSND_IPREEMPH_WARM_MAX]: the scan parallel over time - every lane owns 32 samples and first runs over the
 *            `warm` samples before them from state 0 (from the clip start, where the state is exactly 0, if that is nearer), which leaves
 *            an error <= 2 |w_hh|^warm in its first sample.  The caller's rule: the smallest such warm with 2 |w_hh|^warm <= 2^-25;
 *        PSND_IPREEMPH_SEQ: one lane per clip, exact for any w_hh - for |w_hh| >= 1 and wherever the rule asks for more than WARM_MAX;
 *        PSND_IPREEMPH_AUTO: the kernel applies that rule to *w_hh itself (no host copy of the weight needed, graph-capturable).
 *  psnd_ipreemph_bwd: with d[t] = (1 - y[t]^2) (gy[t] + w_hh d[t+1]), d[T] = 0:  gx[t] = w_ih d[t] (fully overwritten),
 *      gw[0] = sum d[t] x[t] (gradient of w_ih), gw[1] = sum d[t] y[t-1] (of w_hh), over all clips.  Same instances, mirrored in time.
 *      partial : scratch of 2 * 256 * N * ceil(T / PSND_IPREEMPH_SPAN) doubles, every entry used is written first; a second launch adds
 *      them in index order (no atomics: gw is bit-reproducible).
 *  psnd_volnorm_fwd: hop i (start = i * hop, one for every start < L - window) - std[i] = unbiased standard deviation of all B * window
 *      elements wav[:, start : start + window] (two passes in double), out[:, start : stop] = wav[:, start : stop] / (std[i] * inv_gain),
 *      inv_gain = 1 / 10^(target_db / 10); stop = start + hop, for the last hop out_len - the caller applies the reference's tail rule
 *      (models/sound.py volnorm_layout).  wav (B, L), out (B, out_len), std : one float per hop, all fully overwritten.
 *  psnd_volnorm_reverse: the same tiling, out[:, start : stop] = wav[:, start : stop] * (std[i] / gain), gain = 10^(target_db / 10), std
 *      read. */
#define PSND_IPREEMPH_SPAN 8192
#define PSND_IPREEMPH_WARM_MAX 2048
#define PSND_IPREEMPH_SEQ (-1)
#define PSND_IPREEMPH_AUTO (-2)
int psnd_ipreemph_fwd(const float *x, int64_t N, int64_t T, const float *w_ih, const float *w_hh, int warm, float *y,
                      void *stream);
int psnd_ipreemph_bwd(const float *gy, const float *y, const float *x, int64_t N, int64_t T, const float *w_ih,
                      const float *w_hh, int warm, float *gx, double *partial, float *gw, void *stream);
int psnd_volnorm_fwd(const float *wav, int64_t B, int64_t L, int window, int hop, float inv_gain, float *out,
                     int64_t out_len, float *std, void *stream);
int psnd_volnorm_reverse(const float *wav, int64_t B, int64_t L, int window, int hop, float gain, const float *std,
                         float *out, int64_t out_len, void *stream);

/* ---- utils/sound.py: preemphasis / inv_preemphasis (:66-71, scipy.signal.lfilter on the host) and lowpass (:25-35) as one recursive
 *  filter section of order <= 2 on device tensors (psnd_lfilter.hip) ------------------------------------------------------------------
 *  psnd_lfilter: per row of x, y : (N, T) fp32, coefficients already divided by a0:
 *        y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2],  zero state before t = 0  (scipy's lfilter with zi = None).
 *      reverse = 1: the same filter mirrored in time (t+k for t-k, zero state beyond T-1) - the adjoint, i.e. the input gradient.
 *      The recurrence is held as a two-element state (direct form II transposed) in fp64; the coefficients are plain doubles passed by
 *      value, so a call can be captured.  `instance`:
 *        PSND_LFILTER_PARALLEL: an exact scan over time.  A lane walks PSND_LFILTER_CHUNK samples from the zero state; end states combine
 *            as s_out = M^len s_in + r, M = [[-a1, 1], [-a2, 0]], across the lanes of a wave by shuffles, across the waves of a workgroup
 *            through LDS, and across the workgroups of a row (one per PSND_LFILTER_SPAN samples) through `carry` and a launch boundary:
 *            the first launch writes every span's zero-state end state, the second folds the ones before its span and walks again.  No
 *            workgroup waits on another inside a launch.  The caller's rule: this instance whenever every entry of M^PSND_LFILTER_SPAN
 *            is finite (any pole inside or on the unit circle, and outside it as far as the power stays finite);
 *        PSND_LFILTER_SEQ: one lane per row, for every other filter (and for NaN coefficients).
 *      carry : N * psnd_lfilter_spans(T) * 2 doubles of scratch for the parallel instance (every entry read is written first; may be
 *      NULL for PSND_LFILTER_SEQ).  x != y.  N == 0 or T == 0: nothing to do.
 *  psnd_lfilter_spans(T): ceil(T / PSND_LFILTER_SPAN), 0 for T <= 0 (host helper). */
#define PSND_LFILTER_SPAN 8192
#define PSND_LFILTER_CHUNK 32
#define PSND_LFILTER_PARALLEL 0
#define PSND_LFILTER_SEQ 1
int64_t psnd_lfilter_spans(int64_t T);
int psnd_lfilter(const float *x, int64_t N, int64_t T, double b0, double b1, double b2, double a1, double a2, int reverse,
                 int instance, double *carry, float *y, void *stream);

/* ---- sample-rate conversion by a rational factor up / down on device tensors (psnd_resample.hip): what the reference leaves to sox
 *  (scripts/preprocess.py:82-88) and ffmpeg (:32-41).  The definition is scipy.signal.resample_poly's with zero padding -----------------
 *  psnd_resample: per row of x : (N, T) fp32 into y : (N, T_out) fp32, with P = (taps - 1) / 2 and h the `taps` fp32 filter values
 *  (designed in float64 on the host and rounded once; scipy's firwin(2P+1, 1/max(up,down), ('kaiser', 5.0)) * up for P = 10 max(up, down)):
 *        y[n][m] = sum_i x[n][i] g[m down - i up + P],   0 <= m < T_out,  over 0 <= i < T with 0 <= m down - i up + P <= 2P,
 *        g = h (flip 0) or h reversed (flip 1).
 *      The forward conversion is (up, down, flip 0, T_out = psnd_resample_len(T, up, down)).  Its adjoint - the input gradient - is the same
 *      call with up and down exchanged, flip 1, the gradient as x and T_out = the length of the forward input: one kernel, both ways.
 *      T_out is the caller's: outputs that no input reaches are written as zeros.
 *      h is read as given, in natural order (no packed plan): a workgroup of 256 lanes owns PSND_RESAMPLE_TILE consecutive outputs of one
 *      row, keeps g whole in LDS (reversed while loading for flip 1; output m reads g[phi + j up], phi = (m down + P) mod up, and
 *      neighbouring lanes differ in phi by down mod up words) and stages the span of x that its tile reaches through LDS in pieces of
 *      3072 samples.  Products are accumulated in fp32 from the newest input sample to the oldest; no atomics, the same bits every run.
 *      All loads and stores are single dwords: rows may start at any 4-byte boundary.  Every element of y[0 .. N T_out) is written,
 *      nothing else.  x != y.  N == 0 or T_out == 0: nothing to do; T == 0 with T_out > 0 writes zeros (x may then be NULL).
 *      taps must be odd, positive and at most PSND_RESAMPLE_MAX_TAPS (12801: 11.025 kHz <-> 16 / 48 kHz, the widest pair among the
 *      usual audio rates; g and the staged span share 64 KB of LDS); up, down > 0; sizes >= 0.  Bad arguments return PSND_E_ARG (more
 *      than 2^31 - 1 workgroups: PSND_E_SHAPE) before anything is launched.
 *  psnd_resample_len(T, up, down): ceil(T up / down), 0 for T <= 0 or a non-positive factor (host helper). */
#define PSND_RESAMPLE_TILE 1024
#define PSND_RESAMPLE_MAX_TAPS 12801
int64_t psnd_resample_len(int64_t T, int up, int down);
int psnd_resample(const float *x, int64_t N, int64_t T, const float *h, int taps, int up, int down, int flip, float *y, int64_t T_out,
                  void *stream);

/* ---- utils/silence.py: detect_silence (:25-80, pydub's detector on numpy: one x.dot(x) per window start in a Python loop) on device
 *  tensors (psnd_silence.hip) ------------------------------------------------------------------------------------------------------------
 *  Every row x of T_r samples (fp32) on its own; window L >= 1 samples, step s >= 1 samples (the reference's "ms" are sample counts).
 *    Starts.    None if T_r < L; else 0, s, 2s, ... <= T_r - L, plus T_r - L itself when it is no multiple of s.
 *    Decision.  The window at i is silent iff E(i) = sum_{t in [i, i+L)} x[t]^2 <= theta.  theta = L 10^(dB/10), formed in double on the
 *               host and passed by value, so a call can be captured: the reference's rms <= 10^(dB/20).  dB = -inf gives theta = 0: only
 *               windows of exact zeros are silent.  A window that holds a NaN or +-Inf sample is not silent (the reference: nan <= thr is
 *               false), and such a sample changes the decision of no window that does not hold it.
 *    Merging, in the order of silent starts, p = the silent start before: a silent start k opens a new range iff it is the first one, or
 *               k != p + s and k > p + L.  A range is [first start, last start + L].  With s > L grid neighbours still merge across the gap
 *               between them, as in the reference.
 *    Outputs.   count[row] (int32); ranges[row][r][0:2] (int64) for r < count, -1 in the entries r >= count up to `cap`.
 *               psnd_silence_cap(T, L) = floor((T - L) / (L + 1)) + 1 ranges per row always suffice (two range heads are more than L
 *               apart); 0 for T < L.
 *  E is exact to fp64 rounding of a sum of at most L + PSND_SILENCE_BLOCK terms - never a difference of two row-long prefix sums, which
 *  loses a quiet window behind a loud passage.  Three launches, no workgroup waits on another inside one, no atomics:
 *    A  per block of PSND_SILENCE_BLOCK samples of a row, the inclusive fp64 prefix of x^2 restarted at the block's first sample (the last
 *       entry is the block's total) and the int32 prefix of the count of non-finite samples, which enter the fp64 sum as 0;
 *    B  one lane per start: E = tail of the first block + the totals of the whole blocks between + head of the last block (three
 *       non-negative parts), the non-finite count by the same decomposition, one byte per start;
 *    C  one workgroup per row walks the flags in chunks: p is an exclusive prefix maximum of silent starts, range ordinals a prefix sum of
 *       head flags (wave scans by ballots and one shuffle, the four waves meet through LDS, the previous silent start and the ordinal carried from chunk
 *       to chunk); a head of ordinal r > 0 also writes the end of range r - 1, the last end is written behind the walk, then the -1 fill.
 *  lengths : per-row valid lengths (device int64, clamped to [0, T]) or NULL for T everywhere - a zero-padded collated batch as ragged
 *      rows; a row shorter than L has count 0.  scratch : psnd_silence_scratch_bytes(N, T, L, s) bytes, 16-byte aligned (12 per sample and
 *      one per start, rounded up); every entry that is read has been written by the same call.  x may start on any 4-byte boundary.
 *  PSND_E_ARG before anything is launched: L < 1, s < 1, cap < psnd_silence_cap(T, L), NaN theta, N or T < 0, a NULL pointer with
 *  N, T > 0 (more than 2^31 - 1 workgroups: PSND_E_SHAPE).  N == 0 or T == 0: nothing to do.
 *  psnd_silence_starts(T, L, s): the number of window starts of a row of T samples (host helper, as psnd_silence_cap). */
#define PSND_SILENCE_BLOCK 1024
int64_t psnd_silence_cap(int64_t T, int64_t L);
int64_t psnd_silence_starts(int64_t T, int64_t L, int64_t s);
size_t psnd_silence_scratch_bytes(int64_t N, int64_t T, int64_t L, int64_t s);
int psnd_silence_ranges(const float *x, int64_t N, int64_t T, const int64_t *lengths, int64_t L, int64_t s, double theta, void *scratch,
                        int32_t *count, int64_t *ranges, int64_t cap, void *stream);

/* ---- fundamental frequency per frame on device tensors (psnd_pitch.hip): the place of utils/sound.py get_f0 (:38-49), which calls WORLD's
 *  DIO + StoneMask through pyworld.  What is computed here is NOT WORLD: it is YIN (de Cheveigne & Kawahara, JASA 111 (4), 2002), steps
 *  1-5, as written out below; parity with WORLD is unpinned.  Kept of the reference's contract: one value per frame at the times
 *  i hop / sr, T / hop + 1 frames (WORLD's GetSamplesForDIO for frame_period = 1000 hop / sr in exact integers), 0 for an unvoiced frame.
 *  Every row x of T_r samples (fp32) on its own.  Caller's parameters: hop >= 1, W >= tau_max >= tau_min >= 2, threshold > 0, sr > 0
 *  (utils.pitch derives tau_min = max(2, floor(sr / f0_ceil)), tau_max = ceil(sr / f0_floor), W = 2 tau_max).  span = W + tau_max,
 *  H = span / 2 (integer division).
 *    Frames.   F_r = T_r / hop + 1.  Frame i reads u[j] = x[i hop - H + j], j < span; samples outside [0, T_r) are zeros.
 *    1  d(tau) = sum_{j < W} (u[j] - u[j + tau])^2, tau = 1 .. tau_max: the direct sum of squared differences in fp32, j ascending - not
 *       energy minus autocorrelation (it cancels), no running sum from frame to frame.
 *    2  d'(tau) = d(tau) tau / sum_{k = 1 .. tau} d(k); 1 where that sum is 0.
 *    3  t0 = the smallest tau in [tau_min, tau_max] with d'(tau) < threshold.  None: the frame is unvoiced, lag = 0, f0 = 0,
 *       aperiodicity = min d' over that range.
 *    4  t = t0; while t + 1 <= tau_max and d'(t + 1) < d'(t): t = t + 1.
 *    5  if t - 1 >= 1 and t + 1 <= tau_max: y0, y1, y2 = d'(t - 1), d'(t), d'(t + 1), den = y0 - 2 y1 + y2,
 *       off = clamp((y0 - y2) / (2 den), -1/2, 1/2) if den > 0, else 0; otherwise off = 0.  f0 = sr / (t + off), lag = t,
 *       aperiodicity = d'(t).
 *    6  A frame whose span holds a NaN or an Inf is unvoiced with aperiodicity 1, decided by a test of the exponent bits before step 1.
 *    Outputs.  f0, aperiodicity (fp32), lag (int32), each (N, F) with F >= psnd_yin_frames(T, hop); EVERY slot is written: the slots of
 *              row r from F_r on hold f0 = 0, aperiodicity = 1, lag = 0.
 *  lengths : per-row valid lengths (device int64, clamped to [0, T]) or NULL for T everywhere; samples at or behind a row's length are
 *      read as zeros whatever the memory holds (no global read leaves [0, T_r)).  x may start on any 4-byte boundary.
 *  One launch, no scratch, no atomics: a workgroup of 4 waves takes 4 consecutive frames of a row, stages their spans in LDS once (the
 *  union when hop < span, back to back otherwise), one wave per frame, lane l the lags 1 + l + 64 k; the prefix sum of step 2 is a wave
 *  scan in fp32, step 3 a ballot, steps 4-5 a walk over d' in LDS.
 *  Limits: span = W + tau_max <= psnd_yin_max_span() = 6144 (4 spans and 4 rows of d' share the LDS; 48 kHz with a 50 Hz floor is
 *      tau_max = 960, W = 1920, span = 2880; 44.1 kHz down to 22 Hz with W = 2 tau_max fits as well); at most 2^31 - 1 workgroups.
 *  PSND_E_ARG before anything is launched: hop < 1, tau_min < 2, tau_max < tau_min, W < tau_max, span beyond the limit, a NaN or
 *      non-positive threshold or sr, F < psnd_yin_frames(T, hop), N or T < 0, a NULL pointer with N > 0 (x may be NULL when T == 0);
 *      more workgroups than the grid holds: PSND_E_SHAPE.  N == 0: PSND_OK, nothing launched.
 *  psnd_yin_frames(T, hop): T / hop + 1 (0 for T < 0 or hop < 1; host helper). */
int64_t psnd_yin_frames(int64_t T, int64_t hop);
int64_t psnd_yin_max_span(void);
int psnd_yin_f0(const float *x, int64_t N, int64_t T, const int64_t *lengths, int64_t hop, int64_t W, int64_t tau_min, int64_t tau_max,
                float threshold, double sr, float *f0, float *aperiodicity, int32_t *lag, int64_t F, void *stream);

/* ---- time-scale modification of a complex spectrogram on device tensors (psnd_phase_vocoder.hip): the phase vocoder between
 *  STFT.transform_complex and STFT.inverse_complex, what utils.sound.time_stretch / pitch_shift are built on.  The reference reaches such
 *  effects through pysndfx (sox `tempo` / `pitch`, which is WSOLA); what is computed here is the plain phase vocoder of torchaudio's
 *  phase_vocoder and librosa's time_stretch - parity with sox is unpinned.
 *  Inputs.   re, im : fp32 (N, K, F), the frame axis contiguous; X = re + i im.  rate : a double, positive and finite.  frames : one
 *            int64 per batch item n (device), clamped to [0, F], or NULL for F_n = F everywhere; X[n, k, f] counts as 0 for f >= F_n
 *            whatever the memory holds (no global read leaves [0, F_n)).
 *  Per row (n, k) and output frame j = 0, 1, ...:
 *      t_j = (double) j * rate     one IEEE double multiplication, not fused with what follows
 *      i_j = floor(t_j),  alpha_j = t_j - i_j
 *      mag_j = (1 - alpha_j) |X[i_j]| + alpha_j |X[i_j + 1]|
 *      phi_0 = arg X[0],  phi_j = phi_{j-1} + (arg X[i_{j-1} + 1] - arg X[i_{j-1}]),  arg 0 = 0 (either sign of either zero)
 *      Y_j = mag_j (cos phi_j, sin phi_j)
 *  Row n has J_n = psnd_pv_frames(F_n, rate) valid output frames: the number of j >= 0 with (double) j * rate < F_n (counted by that
 *  wording, not a bare ceil(F / rate)).  Outputs yre, yim : fp32 (N, K, J) with J >= psnd_pv_frames(F, rate); EVERY slot is written, the
 *  slots of a row from J_n on hold (0, 0).
 *  Only phi mod 2 pi matters, which makes this the function of the textbook wording (subtract the bin's expected advance
 *  pi hop k / (K - 1), wrap to [-pi, pi], add it back, cumsum): the expected advance cancels modulo a turn, so neither n_fft nor hop is
 *  a parameter.
 *  Freedoms of the implementation: the phase may be accumulated in any way that keeps it to float32 rounding of the single angles over
 *  rows of any length (fp64, a fixed-point fraction of a turn, renormalised complex products); arg may be avoided altogether.  This one
 *  takes atan2f of every element it reads, turns each angle into a 64-bit fixed-point fraction of a turn (2^64 = one turn, exact and
 *  order-independent under integer addition, the modulo is the wrap-around) and sums those.
 *  Non-finite input.  Rows are independent.  In a row that reads a NaN or an Inf - X[i_j] or X[i_j + 1] of some frame j - every output
 *  frame from the first such j on is NaN in both parts (through its own mag or through an earlier phase step: a lost phase must not look
 *  like audio); an element no frame reads (skipped at rate > 1, at or behind F_n) changes nothing; no other row changes by a bit.
 *  One launch, no scratch, no atomics, no host synchronisation; a fixed order of operations: repeated launches agree bit for bit.  A wave
 *  walks one row in passes of psnd_pv_pass() = 64 x 4 consecutive output frames (a lane owns 4 consecutive frames: 16-byte stores), an
 *  in-wave scan of the phase steps with a carry from pass to pass.  Rows are not split (profiles/NOTEBOOK.md has the one-clip figure).
 *  psnd_pv_pass(): the frames per pass, the one size the kernel's seams depend on (host helper; a function, as psnd_yin_max_span, not
 *  a macro: the set of macros of this header is pinned by tests/test_cabi.py).
 *  PSND_E_ARG before anything is launched: rate not positive and finite, N, K or F < 0, J >= 2^31, J < psnd_pv_frames(F, rate), a NULL
 *      pointer with work to do (re / im may be NULL when F == 0, frames always); more than 2^31 - 1 workgroups: PSND_E_SHAPE.
 *      N K == 0 or J == 0: PSND_OK, nothing launched.
 *  psnd_pv_frames(F, rate): host helper, 0 for F <= 0 or a rate that is not positive and finite, INT64_MAX where the count passes 2^53. */
int64_t psnd_pv_pass(void);
int64_t psnd_pv_frames(int64_t F, double rate);
int psnd_phase_vocoder(const float *re, const float *im, int64_t N, int64_t K, int64_t F, const int64_t *frames, double rate, float *yre,
                       float *yim, int64_t J, void *stream);

/* ---- Griffin-Lim on device tensors (psnd_griffinlim.hip): a waveform from a magnitude spectrogram alone, what kernels.griffinlim,
 *  utils.sound.griffinlim and models.sound.GriffinLim are built on.  The definition is torchaudio's functional.griffinlim and librosa's
 *  griffinlim - the fast Griffin-Lim of Perraudin, Balazs and Sondergaard (2013) - on this project's STFT.transform_complex /
 *  inverse_complex.  The reference has no such function: there is no parity to pin.  The two entry points below are the start of the loop
 *  and the phase step between the two transforms; the loop itself lives in kernels.griffinlim.
 *  Inputs.   S = mag : fp32 (N, K, F), the frame axis contiguous, elements e = k F + f of item n at n K F + e.  alpha = momentum /
 *            (1 + momentum) and eps (the loop passes 1e-16) : floats by value.  frames : one int64 per batch item n (device), clamped to
 *            [0, F], or NULL for F_n = F everywhere.
 *  Start.    X0 = S (cos phi, sin phi) for a phase tensor phi of S's shape; X0 = (S, +0) when phi is NULL.
 *  Each of n_iter iterations.
 *      y = inverse_complex(X),  C = transform_complex(y)
 *      t = C - alpha P   componentwise, P the C of the iteration before; in the first iteration (pre and pim NULL) t = C
 *      r = hypot(t_re, t_im)
 *      X = S (t / (r + eps))    the quotient first, then the product with S: |t| near 1e30 does not overflow, t = 0 gives exactly (0, 0),
 *                               and so does S = 0 wherever the quotient is finite
 *      then P = C
 *  End.      y = inverse_complex(X): (F - 1) hop samples.
 *  Ragged items.  Elements at f >= F_n are written as (+0, +0) by both entry points and are never read, whatever the memory holds - of no
 *  input plane.
 *  Convergence measure (optional).  conv[i, n] = sqrt(sum (|C| - S)^2 / sum S^2) over the valid elements of item n in iteration i, 0
 *  where the denominator is 0.  The step writes, when `partial` is given, one pair of fp32 sums per chunk: partial is
 *  (N, psnd_gl_chunks(K, F), 2) with [n, c, 0] = sum (hypot(C_re, C_im) - S)^2 and [n, c, 1] = sum S^2 over the valid elements
 *  c psnd_gl_chunk() <= e < (c + 1) psnd_gl_chunk() of item n (a chunk belongs to one item; a chunk without valid elements holds (0, 0)).
 *  The caller adds the pairs up (kernels.griffinlim: in float64, once, after the last iteration).
 *  Non-finite input: no special rule; it propagates as IEEE arithmetic gives.
 *  Freedoms of the implementation: a fused or unfused multiply-add in t; the device library's hypotf (and sincosf in the start).
 *  Everything else - the subtraction order, the addition of eps, the IEEE division, the product - is as written.  This implementation
 *  takes t = fmaf(-alpha, P, C).
 *  One launch each, no atomics, no scratch beyond `partial`, no host synchronisation; a fixed order of operations: repeated launches agree
 *  bit for bit, `partial` included (a lane adds its elements in ascending order, the lanes of a wave are added by a shuffle tree, the waves of
 *  a workgroup in ascending order).  A workgroup takes one chunk of psnd_gl_chunk() consecutive elements of one item; a lane owns groups of
 *  4 consecutive elements (16-byte loads and stores where the address allows; any 4-byte alignment and any K F are served, a group that
 *  crosses the end of a ragged row or of the item goes element by element).  Five planes read, two written: 28 N K F bytes per step.
 *  Aliasing: xre / xim may be the very buffers pre / pim (each element is read before the lane that owns it writes it); no other two
 *  arguments may overlap.
 *  psnd_gl_chunk(): the elements per workgroup, the one size the kernel's seams depend on (host helper; a function, as psnd_pv_pass, not a
 *  macro: the set of macros of this header is pinned by tests/test_cabi.py).  psnd_gl_chunks(K, F): the chunks per item,
 *  ceil(K F / psnd_gl_chunk()); 0 for K <= 0 or F <= 0.
 *  PSND_E_ARG before anything is launched: N, K or F < 0, exactly one of pre / pim NULL, a NULL pointer with work to do (phase, frames,
 *      partial and the pair pre / pim may be NULL always).  PSND_E_SHAPE: K F >= 2^31, or more than 2^31 - 1 workgroups.
 *      N K F == 0: PSND_OK, nothing launched, no pointer looked at. */
int64_t psnd_gl_chunk(void);
int64_t psnd_gl_chunks(int64_t K, int64_t F);
int psnd_griffinlim_start(const float *mag, const float *phase, int64_t N, int64_t K, int64_t F, const int64_t *frames, float *xre,
                          float *xim, void *stream);
int psnd_griffinlim_step(const float *mag, const float *cre, const float *cim, const float *pre, const float *pim, int64_t N, int64_t K,
                         int64_t F, const int64_t *frames, float alpha, float eps, float *xre, float *xim, float *partial, void *stream);

/* ---- mel to linear magnitude on device tensors (psnd_mel_inverse.hip): what kernels.mel_inverse, models.transforms.InverseMelScale,
 *  LogMelSpectrogram.inverse_mel, utils.sound.mel_to_magnitude / mel_to_wave and models.sound.MelToWave are built on.  Every frame is an
 *  independent non-negative least-squares problem, M equations in K unknowns, solved by a fixed number of FISTA steps (Beck and Teboulle
 *  2009) from a flat-band guess.  torchaudio's InverseMelScale (lstsq) and librosa's mel_to_stft (NNLS by L-BFGS-B) are other algorithms:
 *  the definition below is the contract, there is no parity to pin.
 *  Inputs.   W : (M, K) fp32, finite and >= 0 (a negative or non-finite weight is PSND_E_ARG of the plan builder, not a clamp).
 *            Y = mel : fp32 (N, M, F), the frame axis contiguous.  log_kind in {PSND_LOG_NONE, PSND_LOG_E, PSND_LOG_10}, log_offset.
 *            n_iter >= 0.  frames : one int64 per item n (device), clamped to [0, F], or NULL for F_n = F everywhere.
 *  The plan (host, float64; every sum below adds its terms one after the other in ascending index, products are not fused).
 *      s[m] = sum_k W[m,k];  d[m] = 1 / s[m] if s[m] > 0 else 0 (an empty band drops out of the problem)
 *      A = fp32(d[m] W[m,k]): rows that sum to 1 - the raw Slaney-normalised system is badly scaled from the low bands to the high ones.
 *          Only A is rounded; everything below is formed from the ROUNDED A, in float64.
 *      c[k] = sum_m A[m,k];  cinv[k] = 1 / c[k] if c[k] > 0 else 0
 *      L = max_m sum_k A[m,k] c[k], the largest row sum of A A^T, a bound of its largest eigenvalue because A >= 0 (no eigen-solver:
 *          the host code and numpy get it to the bit);  step = 1 / L, or 0 if L = 0
 *      beta_i = (t_{i-1} - 1) / t_i,  t_0 = 1,  t_i = (1 + sqrt(1 + 4 t_{i-1}^2)) / 2,  i = 1 .. n_iter_max; in float64, stored as fp32
 *      The kernel takes d, cinv and step rounded to fp32.
 *  Each valid frame (m and k run over all filters and bins; the vectors are the frame's own).
 *      lin[m] = Y (LOG_NONE), exp(Y) - log_offset (LOG_E), 10^Y - log_offset (LOG_10);   b[m] = d[m] max(lin[m], 0)
 *      x_0[k] = cinv[k] sum_m A[m,k] b[m]   (the flat-band guess);   z = x_0
 *      for i = 1 .. n_iter:   r = A z - b;   g = A^T r;   x_i = max(z - step g, 0);   z = x_i + beta_i (x_i - x_{i-1})
 *      out = x_{n_iter}, (N, K, F).   resid (optional, (N, F)) = sqrt(sum_m r[m]^2 / sum_m b[m]^2) with r = A x_{n_iter} - b, 0 where b = 0.
 *  What follows.  A bin no filter reaches (c[k] = 0) is exactly 0 at every iteration.  Frames f >= F_n are never read, whatever the
 *  memory holds, and come out as 0 (out and resid).  Frames never interact: a non-finite value in a frame may make that frame's output
 *  anything (max(NaN, 0) is 0 here), and leaves every other frame's bits as they are.
 *  Freedoms of the implementation: fused or unfused multiply-adds, the device library's expf / exp10f / sqrtf.  The order of every sum
 *  (ascending m or k over the band from the first to the last non-zero weight) is fixed: repeated launches agree bit for bit, and a
 *  frame's bits depend on nothing but its own column of Y - not on f, n, N, F or its neighbours.
 *  The plan, in 4-byte words: a header of 32 words {magic, M, K, n_iter_max, weights in the row bands, weights in the column bands,
 *  step as fp32, 0, then the word offsets of d fp32[M], cinv fp32[K], beta fp32[psnd_mel_inverse_max_iter()], the row bands (per filter
 *  {first bin | length << 16, offset into the row weights}), the column bands (per bin {first filter | length << 16, offset}), the row
 *  weights, the column weights, A fp32 (M, K) dense, the float64 block {step, L, d[M], cinv[K]}, and the word count}.  One launch, a
 *  workgroup owns psnd_mel_inverse_tile(M, K) consecutive frames of one item and keeps x, z, r and b in LDS for all iterations; no scratch,
 *  no atomics, no host synchronisation.  psnd_mel_inverse_tile: the frames per workgroup, the one size the kernel's seams depend on (a
 *  function, as psnd_gl_chunk, not a macro); 0 outside the sizes served.
 *  PSND_E_UNSUPPORTED (psnd_last_error names the limit): M > 256, K > 2049, n_iter or n_iter_max > psnd_mel_inverse_max_iter();
 *      psnd_mel_inverse_plan_bytes returns 0 there.  PSND_E_ARG: a null pointer with work to do, sizes <= 0, a bad log_kind, a bad weight.
 *      PSND_E_SHAPE: K F >= 2^31 or more than 2^31 - 1 workgroups.  N F == 0: PSND_OK, nothing launched.  What the host cannot see (the
 *      plan lives on the device) - memory that is no plan (the magic word), a plan built for another (M, K), n_iter above the n_iter_max
 *      the plan was built with - is found by the launch itself from the first four words of the plan: it reads nothing else of it and
 *      fills out and resid with NaN. */
int psnd_mel_inverse_tile(int M, int K);
int psnd_mel_inverse_max_iter(void);
size_t psnd_mel_inverse_plan_bytes(int M, int K);
int psnd_mel_inverse_plan_build(int M, int K, const float *mel_filter_host, int n_iter_max, void *plan_host);
int psnd_mel_inverse(const float *mel, int64_t N, int64_t F, int M, int K, const void *plan, int log_kind, float log_offset, int n_iter,
                     const int64_t *frames, float *out, float *resid, void *stream);

/* ---- loudness, plain levels and gain on device tensors (psnd_loudness.hip): the level normalisation of the reference's preprocessing
 *  (scripts/preprocess.py:32-41 runs every file through ffmpeg-normalize on the host).  What is computed is ITU-R BS.1770-4 / EBU R128
 *  integrated loudness as written out here; parity with ffmpeg's numbers is unpinned.
 *  A programme is C >= 1 channels of T_r samples (fp32) at rate sr: rows n C .. n C + C - 1 of x : (N C, T).  Every programme on its own.
 *    1  K-weighting.  Two sections of order 2 in series (shelf, then high-pass), each y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1]
 *       - a2 y[t-2] with zero state before t = 0, in fp64.  The ten coefficients are formed on the host in double for the given sr and passed
 *       by value, so a call can be captured:
 *         shelf      K = tan(pi f0 / sr), f0 = 1681.974450955533, Q = 0.7071752369554196, Vh = 10^(3.999843853973347 / 20),
 *                    Vb = Vh^0.4996667741545416, a0 = 1 + K/Q + K^2, b = [(Vh + Vb K/Q + K^2), 2 (K^2 - Vh), (Vh - Vb K/Q + K^2)] / a0,
 *                    a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0]
 *         high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, b = [1, -2, 1], a = [1, 2 (K^2 - 1) / a0, (1 - K/Q + K^2) / a0] with
 *                    its own K and a0
 *       At 48 kHz: b = 1.53512485958697, -2.69169618940638, 1.19839281085285, a1, a2 = -1.69065929318241, 0.73248077421585; high-pass
 *       a1, a2 = -1.99004745483398, 0.99007225036621 (the table of BS.1770, reproduced to 1e-13).
 *    2  Blocks.  Block length B and hop H in samples, 1 <= H <= B, from the caller (the wrappers: B = round(0.4 sr), H = B / 4 rounded
 *       down).  A row has J_r = (T_r - B) / H + 1 complete blocks, none if T_r < B.  z[j] = sum_c G_c (1/B) sum_{t in [jH, jH + B)} y_c[t]^2:
 *       an fp64 sum of at most B + (one span) terms in a fixed order, never a difference of row-long prefixes.  weights: C doubles on the
 *       HOST, read during the call and passed on by value, or NULL for G = 1, 1, 1, 1.41, 1.41 (C <= 5).
 *    3  Gates, in the energy domain in fp64.  Ja = {j : z[j] > 10^((-70 + 0.691) / 10)}; Gamma = 0.1 mean_{Ja} z;
 *       Jg = {j in Ja : z[j] > Gamma}; L = -0.691 + 10 log10(mean_{Jg} z), rounded once to fp32.  Ja empty (J_r = 0 included): L = -inf.
 *       A programme that holds a non-finite sample before its length (in a complete block or not) has L = NaN and NaN in its J_r entries
 *       of `blocks`; it changes no other programme's result.
 *    4  Outputs.  lufs[N] fp32; blocks[N][Jmax] fp32 or NULL, Jmax = psnd_loudness_blocks(T, B, H): the z[j], 0 behind J_r; gain[N] fp32
 *       or NULL: 10^((target - L) / 20) of the fp32 L, exactly 1 where L is -inf, NaN or +inf.
 *  psnd_loudness: an exact time-parallel scan over both sections at once (state of four doubles, end states combine through the powers of
 *  the 4 x 4 block-triangular matrix of the cascade: lanes by shuffles, waves through LDS, the spans of psnd_loudness_span() samples of a
 *  row through a carry array and a launch boundary).  The filtered signal is never written: the second walk squares it in registers into
 *  pieces cut at the multiples of H (and at those plus B mod H, where that is not 0), one fp64 partial per (row, span, piece), each stored
 *  once; the last launch, one workgroup per programme, adds the pieces of a block across spans and channels in ascending order and runs
 *  the two gated means as fixed-order reductions.  At most three launches, no atomics, no workgroup waits on another, nothing read back
 *  by the host, the same bits on every run.
 *    lengths : per-PROGRAMME valid lengths (device int64, N entries, clamped to [0, T]) or NULL.  x may start on any 4-byte boundary.
 *    scratch : psnd_loudness_scratch_bytes(N, C, T, B, H) bytes, 16-byte aligned; every entry that is read has been written by the same call.
 *  psnd_row_level: per programme rms_db = 10 log10(mean x^2) over its C rows (fp64 sum in a fixed order), peak_db = 20 log10(max |x|), and
 *    gain = 10^((target - level) / 20) of the rms (of_peak = 0) or the peak (of_peak = 1); any of the three outputs may be NULL.  No samples
 *    or digital silence: -inf and gain 1.  A non-finite sample: NaN, NaN and gain 1.  One launch, no atomics.
 *  psnd_gain_rows: y[n][t] = x[n][t] gain[n / C] for t before the programme's length, y = x behind it; x == y is allowed.
 *  PSND_E_ARG before anything is launched: B < 1, H < 1, H > B, C < 1, a non-finite coefficient, weight or target, C > 5 without weights,
 *  N or T < 0, a NULL pointer with work to do; PSND_E_UNSUPPORTED: C > psnd_loudness_max_channels(); PSND_E_SHAPE: more than 2^31 - 1
 *  workgroups.  N == 0 or T == 0: nothing to do.  psnd_loudness_span, psnd_loudness_max_channels, psnd_loudness_blocks and
 *  psnd_loudness_scratch_bytes are host helpers (functions, as psnd_pv_pass, not macros). */
int64_t psnd_loudness_span(void);
int64_t psnd_loudness_max_channels(void);
int64_t psnd_loudness_blocks(int64_t T, int64_t B, int64_t H);
size_t psnd_loudness_scratch_bytes(int64_t N, int64_t C, int64_t T, int64_t B, int64_t H);
int psnd_loudness(const float *x, int64_t N, int64_t C, int64_t T, const int64_t *lengths, double sb0, double sb1, double sb2, double sa1,
                  double sa2, double hb0, double hb1, double hb2, double ha1, double ha2, int64_t B, int64_t H, const double *weights,
                  double target, void *scratch, float *lufs, float *blocks, float *gain, void *stream);
int psnd_row_level(const float *x, int64_t N, int64_t C, int64_t T, const int64_t *lengths, int of_peak, double target, float *rms_db,
                   float *peak_db, float *gain, void *stream);
int psnd_gain_rows(const float *x, int64_t N, int64_t C, int64_t T, const int64_t *lengths, const float *gain, float *y, void *stream);

/* ---- separation metrics on device tensors (psnd_separation.hip): SNR, SI-SDR and SD-SDR (Le Roux et al., "SDR - half-baked or well
 *  done?") as values and as a loss, with permutation-invariant matching (PIT), their gradient, and mixing at a wanted SNR.  The
 *  reference names the tasks (VoiceBank, DSD100 / MUSDB18 / MedleyDB, make_background_numpy of scripts/preprocess.py) and has no metric.
 *  An item b of B holds S >= 1 estimates e_i and S targets s_j: est, target : (B, S, T) fp32, row-contiguous, rows may start on any
 *  4-byte boundary.  Only samples t < L_b count: lengths is a device int64[B], clamped to [0, T], or NULL for L_b = T.
 *    1  Moments.  fp64 sums in a fixed order over t < L:  Se_i = sum e_i, Ss_j = sum s_j, See_i = sum e_i^2, Sss_j = sum s_j^2,
 *       Ses_ij = sum e_i s_j for every pair.  A product of two fp32 values is exact in fp64: the only rounding is in the additions.
 *       With zero_mean = 1 the centred moments are formed from these, ee = See - Se^2 / L, ss = Sss - Ss^2 / L, es = Ses - Se Ss / L;
 *       with zero_mean = 0, ee = See, ss = Sss, es = Ses.  L = 0 leaves them 0; a centred ee or ss below 0 (rounding, on a constant row) is 0.
 *    2  Pair value of (i, j) from ee = ee_i, ss = ss_j, es = es_ij with eps >= 0 passed by value (the wrappers: fp32 machine epsilon,
 *       torchmetrics' choice).  kind is a plain int, no macro:
 *         0 snr     N = ss - 2 es + ee;                                       v = 10 log10((ss + eps) / (N + eps))
 *         1 si_sdr  a = (es + eps) / (ss + eps); Tg = a^2 ss; N = Tg - 2 a es + ee;   v = 10 log10((Tg + eps) / (N + eps))
 *         2 sd_sdr  a and Tg as above;           N = ss - 2 es + ee;          v = 10 log10((Tg + eps) / (N + eps))
 *       N is clamped at 0 from below before eps is added.  All in fp64; v is rounded once to fp32.  (0 / 0 with eps = 0 reads NaN.)
 *    3  Matching.  pit = 0: estimate i is matched with target i (only the diagonal is formed unless `pair` is asked for).  pit = 1: the
 *       permutation p that maximises sum_i v[i][p(i)] - the fp32 values, added in fp64 in ascending i - among the S! permutations walked
 *       in lexicographic order; a later one wins only by a strictly larger sum, so ties go to the lexicographically first.
 *       S <= psnd_sep_max_sources() (4).  An item with a non-finite sample before its length gets NaN in all its values (its row of
 *       `pair` included) and the identity permutation; it changes no other item's result.
 *    4  Outputs.  value[B][S] fp32: v[i][p(i)];  perm[B][S] int32: p;  pair[B][S][S] fp32 or NULL: the whole matrix v[i][j];
 *       loss[1] fp32 or NULL: -(1 / (B S)) sum value, added in fp64 in a fixed order;  nan_flag[1] fp32 or NULL: 1 where that sum is NaN,
 *       else 0, written by the launch that forms the loss;  stats: psnd_sep_stats_doubles(B, S) doubles owned by the caller, kept for the
 *       backward - per item S^2 + 4 S + 2 of them: Se[S], Ss[S], See[S], Sss[S], Ses[S][S], L, and 1.0 where the item is non-finite.
 *  psnd_sep_metric_fwd.  Launch 1: a workgroup reads one span of psnd_sep_span() samples of all 2 S rows of an item once - a scalar head
 *  up to the first 16-byte boundary of the item's first estimate row, 16-byte loads, a scalar tail; a row whose start is not congruent
 *  to that row's modulo 16 bytes is read by the same 16-byte loads at 4-byte aligned addresses - with the S^2 + 4 S accumulators of a
 *  lane in registers as fp64; lanes reduce by shuffles, waves through LDS, and one partial per (item, span, moment) is stored exactly
 *  once.  Launch 2, one wave per item: the partials in ascending span order, the pair matrix, the permutations, value / perm / pair /
 *  stats.  Launch 3 (only where loss or nan_flag is asked for): the loss and the flag.  At most three launches, no atomics, no workgroup
 *  waits on another, nothing read back by the host, the same bits on every run of the same call (the order of the additions depends on
 *  the addresses modulo 16 bytes, on T and on the lengths, on nothing else).  The longest serial run of additions is span / 256 + 1
 *  in a lane, the tree above it is 6 + 3 deep, and the spans of a row follow serially: m + d = ceil(T / span) + 42.
 *    scratch : psnd_sep_scratch_bytes(B, S, T) bytes, 8-byte aligned; every entry that is read has been written by the same call.
 *  psnd_sep_metric_bwd.  One elementwise launch.  With G[b][i] = g_value[b][i] - g_loss / (B S) (either pointer may be NULL, not both;
 *  g_loss is a device fp32 scalar) it writes g_est[b][i][t] = G (A e_i[t] + Bc s_p(i)[t] + C) and, where g_target is not NULL,
 *  g_target[b][p(i)][t] = G (A' e_i[t] + B' s_p(i)[t] + C') for t < L and exactly 0 behind L: every element once.  L is the one the
 *  forward kept in `stats`.  The six coefficients
 *  are the derivatives of the formulas of 2 (eps takes part in a; the clamp passes the gradient where N >= 0) formed in fp64 from `stats`
 *  and `perm` in device memory; C, C' != 0 only with zero_mean.  The rows of a non-finite item get NaN before L.
 *  Mixing at an SNR (torchaudio's add_noise).  psnd_snr_gain: g[r] = sqrt(sum x^2 / sum z^2) 10^(-snr / 20) over t < L_r in fp64,
 *  rounded to fp32, from launch 1 above with S = 1 plus one small launch; snr is a device fp32[R] (snr_n = R) or one device value
 *  (snr_n = 1).  g = 0 where sum z^2 = 0, where sum x^2 = 0, or where either row holds a non-finite sample before L.
 *  scratch: psnd_sep_scratch_bytes(R, 1, T).  psnd_mix_rows: y[r][t] = fmaf(g[r], z[r][t], x[r][t]) for t < L_r and y = x behind it (and everywhere where g[r] = 0);
 *  x == y is allowed: the sibling of psnd_gain_rows.
 *  PSND_E_ARG before anything is launched: a kind outside 0..2, zero_mean or pit outside 0..1, eps < 0 or not finite, S < 1, B or T < 0,
 *  snr_n that is neither 1 nor R, a NULL pointer with work to do, a scratch that is not 8-byte aligned; PSND_E_UNSUPPORTED:
 *  S > psnd_sep_max_sources(); PSND_E_SHAPE: more than 2^31 - 1 workgroups.  B == 0 or T == 0 (R == 0 for the mixing pair): nothing is
 *  launched and no output is touched, except that a requested loss is set to 0 - the empty sum - and a requested nan_flag to 0, by a
 *  memset on the stream.  psnd_sep_span, psnd_sep_max_sources, psnd_sep_scratch_bytes and psnd_sep_stats_doubles are host helpers
 *  (functions, not macros).
 *  Out of scope: BSS-eval SDR with a distortion filter (mir_eval, torchmetrics' signal_distortion_ratio), PESQ / STOI, Hungarian
 *  matching for large S, multichannel items. */
int64_t psnd_sep_span(void);
int64_t psnd_sep_max_sources(void);
size_t psnd_sep_scratch_bytes(int64_t B, int64_t S, int64_t T);
int64_t psnd_sep_stats_doubles(int64_t B, int64_t S);
int psnd_sep_metric_fwd(const float *est, const float *target, int64_t B, int64_t S, int64_t T, const int64_t *lengths, int kind,
                        int zero_mean, double eps, int pit, void *scratch, double *stats, float *value, int *perm, float *pair, float *loss,
                        float *nan_flag, void *stream);
int psnd_sep_metric_bwd(const float *est, const float *target, int64_t B, int64_t S, int64_t T, int kind, int zero_mean, double eps,
                        const double *stats, const int *perm, const float *g_loss, const float *g_value, float *g_est, float *g_target,
                        void *stream);
int psnd_snr_gain(const float *x, const float *z, int64_t R, int64_t T, const int64_t *lengths, const float *snr, int64_t snr_n,
                  void *scratch, float *gain, void *stream);
int psnd_mix_rows(const float *x, const float *z, int64_t R, int64_t T, const int64_t *lengths, const float *gain, float *y, void *stream);

/* ---- fp32 instance of the Conv1d / ConvTranspose1d stack (models/vocoders/hifi_gan.py:32-147 computes its convolutions in fp32) -------
 *  A convolution = psnd_linear1x1_fwd (exact fp32 matrix-core GEMM) over the unfolded input
 *      col[n][ci * k + j][t] = act(x[n][ci][src]),  s' = t * stride + j * dil - pad,  src = s' / up  (0 where s' < 0, s' % up != 0 or src >= T),
 *  act(v) = v > 0 ? v : slope * v (slope 1: none) - the leaky-relu in front of every ResBlock conv (hifi_gan.py:58-61, 86-87).
 *  Conv1d(k, dilation d, padding p): stride 1, up 1, pad p, To = T + 2 p - d (k - 1);  ConvTranspose1d(k, stride u, padding p): up u,
 *  pad k - 1 - p, taps flipped by the caller, To = (T - 1) u - 2 p + k (hifi_gan.py:107-110).  x (N, C, T), col (N, C * k, To) fp32.
 *  psnd_col2im_f32 is the adjoint: gx (N, C, T) from gcol, times act'(x) (x may be NULL when slope == 1). */
int psnd_im2col_f32(const float *x, int64_t N, int C, int64_t T, int k, int dil, int pad, int stride, int up, int64_t To, float slope,
                    float *col, void *stream);
int psnd_col2im_f32(const float *gcol, const float *x, int64_t N, int C, int64_t T, int k, int dil, int pad, int stride, int up, int64_t To,
                    float slope, float *gx, void *stream);

/* ---- data/dataset.py:196-250, SpeechDataLoader.pad_collate_fn on the audio column, device side --------------------
 *  flat : the batch's clips back to back (device, fp32); offs[n], lens[n] : start / length of clip n in flat (device
 *  int64).  out : (N, Tmax) fp32 = clip n zero-padded (or cut) to Tmax;  mask (may be NULL) : (N, Tmax) fp32, 1 on valid
 *  samples and 0 on padding - the reference's np.ones_like(item) after zero padding (dataset.py:70-71, 88-89). */
int psnd_pad_collate(const float *flat, const int64_t *offs, const int64_t *lens, int64_t N, int64_t Tmax, float *out,
                     float *mask, void *stream);

/* ---- SpectrogramMasker.forward (models/transforms.py:409-416): wave-level mask (N, T) fp32 -> frame-level mask (N, F) fp32,
 *  F = psnd_frame_mask_frames(T, win, hop) = (T + 2 (win / 2) - win) / hop + 1: out[n][f] = ceil(mean over frame f of the mask padded with
 *  win / 2 ones in front and win / 2 zeros behind) - the reference's constant-weight Conv1d + ceil without a library convolution. */
int64_t psnd_frame_mask_frames(int64_t T, int win, int hop);
int psnd_frame_mask(const float *mask, int64_t N, int64_t T, int win, int hop, float *out, void *stream);

/* bf16 communication image of a flat fp32 gradient bucket (pytorch_sound_amd/distributed.py, FlatGradReducer(comm_dtype=bfloat16); the reference
 * has no distributed code): dst[i] = bf16(src[i] * scale), round to nearest even / dst[i] = float(src[i]) * scale.  n % 8 == 0. */
int psnd_grad_pack_bf16(const float *src, void *dst, int64_t n, float scale, void *stream);
int psnd_grad_unpack_bf16(const void *src, float *dst, int64_t n, float scale, void *stream);
/* ---- the optimizer step of Trainer.train (trainer.py:215-216) for Adam / AdamW: one launch over all tensors ---------
 *  table : n_tensors records {float *p; const float *g; float *m; float *v; float *step; int64 numel} (device,
 *      psnd_adam_table_bytes() each); the work list: workgroup b updates elements [chunk_off[b], chunk_off[b] +
 *      psnd_adam_chunk()) of tensor chunk_tensor[b] (device arrays, built once per parameter set by the caller).
 *  torch.optim.Adam semantics (amsgrad / maximize off): step += 1; m, v moments; p -= lr / (1 - b1^step) * m /
 *      (sqrt(v) / sqrt(1 - b2^step) + eps); weight_decay as L2 (decoupled = 0) or AdamW (decoupled = 1).
 *      Hyper-parameters are doubles: 1 - beta and the bias corrections are formed in double, as torch does.
 *  found_inf (device, may be NULL): non-zero skips the whole update including the step count (AMP protocol);
 *  grad_scale (device, may be NULL): gradients are divided by it;  corr : 2 * n_tensors floats of device scratch (the
 *      bias corrections, formed in double by a first tiny launch that also advances the step counts).
 *  Trainer.clip_grad (trainer.py:184-191) folded into the same pass: clip_value > 0 clamps every (scaled) gradient element to
 *      [-clip_value, clip_value] (`p.grad.clamp`), clip_coef (device, may be NULL) then multiplies it (`clip_grad_norm_`'s factor,
 *      from psnd_grad_sumsq).  The gradients in memory are left as they are.
 *  psnd_grad_sumsq: the global norm over the SAME table / work list: *sumsq (+)= sum clamp(g / grad_scale, +-clip_value)^2 in double
 *      (partial: n_chunks doubles of device scratch, summed in index order: deterministic), coef[0] = min(1, max_norm / (norm + 1e-6))
 *      (1 when max_norm = 0), coef[1] = norm; accumulate != 0 adds to *sumsq (second and later parameter groups). */
int64_t psnd_adam_chunk(void);
int64_t psnd_adam_table_bytes(void);
int psnd_adam_step(const void *table, int n_tensors, const int *chunk_tensor, const int64_t *chunk_off, int64_t n_chunks,
                   double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                   const float *found_inf, const float *grad_scale, float *corr, float clip_value, const float *clip_coef,
                   void *stream);
/* psnd_adam_step + a host-visible record of the step's skip flag: flag_log = a pinned, device-mapped int ring of {flag, seq} pairs (or NULL);
 * the launch writes flag_log[2 slot] = (found_inf != 0) and then, behind a system-scope fence, flag_log[2 slot + 1] = log_seq.  The host
 * polls the sequence number: no device-to-host copy, no event (Trainer's NaN log line, trainer.py:205-207). */
int psnd_adam_step_logged(const void *table, int n_tensors, const int *chunk_tensor, const int64_t *chunk_off, int64_t n_chunks,
                          double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                          const float *found_inf, const float *grad_scale, float *corr, float clip_value, const float *clip_coef,
                          int *flag_log, int log_slot, int log_seq, void *stream);
/* psnd_adam_step_logged for a Trainer with an LR scheduler whose steps are still in flight (a skipped step must not advance the schedule,
 * trainer.py:211-214, and the host learns of a skip only later): the learning rate is chosen ON THE DEVICE.  lr_ring = rows x n_groups
 * floats in pinned, device-mapped host memory, row j = the rates of all parameter groups after j successful steps; the launch reads
 * good = *good_count (device int) and uses lr_ring[(good % rows) * n_groups + group] in the step size and in AdamW's decay factor.  bump != 0
 * (one launch per step: its last parameter group's): a step that is not skipped then stores good + 1.  A skipped step reads neither ring nor
 * counter.  corr: 2 * n_tensors + 1 floats.  NULL ring or counter, rows <= 0, group outside [0, n_groups): PSND_E_ARG, nothing launched.
 * The rate is out of reach of an argument check: where psnd_adam_step refuses lr < 0 or NaN, this launch uses whatever the ring holds - the
 * caller checks what it writes there (Trainer does: a schedule that yields a negative or NaN rate raises before the row is written). */
int psnd_adam_step_sched(const void *table, int n_tensors, const int *chunk_tensor, const int64_t *chunk_off, int64_t n_chunks,
                         double beta1, double beta2, double eps, double weight_decay, int decoupled,
                         const float *found_inf, const float *grad_scale, float *corr, float clip_value, const float *clip_coef,
                         int *flag_log, int log_slot, int log_seq, const float *lr_ring, int rows, int n_groups, int group,
                         int *good_count, int bump, void *stream);
int psnd_grad_sumsq(const void *table, int n_tensors, const int *chunk_tensor, const int64_t *chunk_off, int64_t n_chunks,
                    float clip_value, const float *grad_scale, int accumulate, float max_norm, double *partial, double *sumsq,
                    float *coef, void *stream);

/* ---- PQMF (models/transforms.py:492-560), polyphase --------------------------------------------------------------
 *  filt : (subbands, taps + 1) fp32 (analysis_filter / synthesis_filter of the module), taps even, P = taps / 2.
 *  psnd_pqmf_analysis : x (B, T) -> out (B, subbands, T / subbands):  out[b][k][m] = scale * sum_j F[k][j] x[b][m S + j - P]
 *      = F.conv1d(pad(x), analysis_filter) followed by the stride-S pick (transforms.py:541-542), zeros outside the signal.
 *  psnd_pqmf_synthesis: x (B, subbands, M) -> y (B, T_out), T_out = M * subbands for the module's synthesis (the adjoint of an
 *      analysis over T samples asks for T_out = T: the tail samples past M * subbands still reach the last frames):
 *      y[b][t] = scale * sum_k sum_{j: (t + j - P) % S == 0} F[k][j] x[b][k][(t + j - P) / S]
 *      = zero-stuffing conv_transpose1d (x S) + F.conv1d(pad(.), synthesis_filter) (transforms.py:552-553) with scale = S.
 *  flip = 1 reverses the taps: each op is then the adjoint of the other (the backward passes). */
int psnd_pqmf_analysis(const float *x, const float *filt, int64_t B, int64_t T, int subbands, int taps, int flip, float scale,
                       float *out, void *stream);
int psnd_pqmf_synthesis(const float *x, const float *filt, int64_t B, int64_t M, int64_t T_out, int subbands, int taps, int flip,
                        float scale, float *y, void *stream);

/* ---- LearnableSTFT (models/transforms.py:104-203): the trainable analysis / synthesis filterbank, exact fp32 (v_mfma_f32_32x32x2_f32) -------
 *  The reference runs F.conv1d / F.conv_transpose1d of the (C, 1, n) basis times the window with stride hop.  Here the frames are a
 *  strided view of the waveform (tap stride 1, frame stride hop): no unfolded (N, n, F) tensor exists.  basis (C, n), window (n) fp32; the
 *  product basis[c][m] * window[m] is rounded to fp32 before it is multiplied, as the reference's `basis * fft_window` is.
 *  psnd_lstft_analysis: spec[z][c][f] = sum_m basis[c][m] window[m] x[z][f hop + m];  x (N, Lx) already padded, F = (Lx - n) / hop + 1,
 *      spec (N, C, F).  mag, phase (N, C / 2, F), both or neither (NULL): mag = sqrt(re^2 + im^2), phase = atan2(im, re) with re = rows
 *      [0, C / 2) and im = rows [C / 2, C) of spec (the reference's chunk(2, 1)), one element pass behind the product; C even then.
 *      transform (:165-178), and the input gradient of inverse (basis = inverse_basis).
 *  psnd_lstft_mag_bwd: gspec (N, C, F) = [gmag re / mag ; gmag im / mag] from spec, mag, gmag (N, C / 2, F).  A bin with mag == 0 gives
 *      (gmag / 0) * 0 = NaN, as autograd of sqrt does and psnd_stft_bwd does.
 *  psnd_lstft_synthesis: y[z][s] = mult[s] * sum_c sum_f g[z][c][f] basis[c][s - f hop] window[s - f hop]  (0 <= s - f hop < n);
 *      = conv_transpose1d(g, (basis * window)[:, None, :], stride=hop).  g (N, C, F), y (N, Ly) with Ly >= n + hop (F - 1); samples
 *      behind the last frame are written as zeros.  mult (Ly) or NULL: a per-sample factor applied in the epilogue (inverse's envelope
 *      division and n / hop scale, :180-203).  Gather (polyphase) form, s = q hop + r: the reduction runs over (j, c) with tap j hop + r
 *      and frame q - j, phases r along the rows and hop blocks q of all clips along the columns of the product - every sample is written
 *      once: no atomics, no zero-fill launch, the same bits from run to run.  hop need not divide n.
 *      inverse, and the waveform gradient of transform (basis = forward_basis).
 *  psnd_lstft_basis_grad: gb[c][m] = window[m] * sum_{z, f} g[z][c][f] x[z][f hop + m];  g (N, C, F), x (N, Lx), F <= (Lx - n) / hop + 1,
 *      gb (C, n).  Partial sums over clip chunks x frame parts go into S = psnd_lstft_wgrad_slabs(N, C, n, F) slabs gb_part
 *      (S * C * n floats, caller's) that are added in a fixed order: bit-reproducible.  forward_basis: g = the gradient of spec, x = the
 *      padded waveform; inverse_basis: g = the spectrum inverse synthesised from, x = the gradient of the full-length y (Lx = n + hop (F - 1)).
 *  PSND_E_ARG without touching the device: hop <= 0, n < 2, rows shorter than n, a NULL required pointer, odd C with mag / phase;
 *  PSND_E_UNSUPPORTED: index ranges the 32-bit tile arithmetic does not cover. */
int psnd_lstft_analysis(const float *x, const float *basis, const float *window, int64_t N, int64_t Lx, int C, int n, int hop, float *spec,
                        float *mag, float *phase, void *stream);
int psnd_lstft_mag_bwd(const float *spec, const float *mag, const float *gmag, int64_t N, int C, int64_t F, float *gspec, void *stream);
int psnd_lstft_synthesis(const float *g, const float *basis, const float *window, const float *mult, int64_t N, int C, int64_t F, int n,
                         int hop, int64_t Ly, float *y, void *stream);
int64_t psnd_lstft_wgrad_slabs(int64_t N, int C, int n, int64_t F);
int psnd_lstft_basis_grad(const float *g, const float *x, const float *window, int64_t N, int64_t Lx, int C, int n, int hop, int64_t F,
                          float *gb_part, float *gb, void *stream);

/* ---- F.l1_loss (reduction 'mean') as used by the training recipes' spectral losses --------------------------------
 *  psnd_l1_loss_fwd: out[0] = mean |a - b| over n fp32 elements; part: psnd_l1_loss_blocks(n) doubles of scratch (one partial
 *      per 16384-element chunk, summed in a fixed order by a second tiny launch: bit-reproducible).
 *  psnd_l1_loss_bwd: ga = g[0] * sign(a - b) / n, gb = -ga (either NULL); g = device pointer to the upstream gradient. */
int64_t psnd_l1_loss_blocks(int64_t n);
/* masked L1 of padded batches (data/dataset.py:196-250 pads the clips of a batch to its longest): a, b (N,C,T) fp32, frame_weight (N,T)
 * fp32 (1 = the frame holds signal): out[0] = sum |a - b| w / (C sum w); part: 2 * psnd_masked_l1_blocks(N*C*T) doubles of scratch;
 * inv_den[0] = 1 / (C sum w) is kept for the backward: ga = g[0] * sign(a - b) * w * inv_den, gb = -ga (either NULL). */
int64_t psnd_masked_l1_blocks(int64_t n);
int psnd_masked_l1_fwd(const float *a, const float *b, const float *frame_weight, int64_t N, int C, int64_t T, double *part, float *out,
                       float *inv_den, void *stream);
int psnd_masked_l1_bwd(const float *a, const float *b, const float *frame_weight, int64_t N, int C, int64_t T, const float *g,
                       const float *inv_den, float *ga, float *gb, void *stream);
int psnd_l1_loss_fwd(const float *a, const float *b, int64_t n, double *part, float *out, void *stream);
int psnd_l1_loss_bwd(const float *a, const float *b, int64_t n, const float *g, float *ga, float *gb, void *stream);
/* a weighted sum of up to 4 mean-L1 terms as ONE scalar (a recipe's `l1(a, b) + 0.5 * l1(c, d)`): out[0] = sum_i w[i] * mean|a[i] - b[i]|;
 * a, b, n, w: HOST arrays of `terms` entries (read during the call); part: sum_i psnd_l1_loss_blocks(n[i]) doubles of scratch.
 * psnd_l1_loss_bwd_w: the backward of one term, ga = weight * g[0] * sign(a - b) / n. */
int psnd_l1_loss_sum_fwd(const float *const *a, const float *const *b, const int64_t *n, const double *w, int terms, double *part,
                         float *out, void *stream);
int psnd_l1_loss_bwd_w(const float *a, const float *b, int64_t n, const float *g, double weight, float *ga, float *gb, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSND_H */
