// psnd_sound.hip - the two sequential utilities of pytorch_sound/models/sound.py on gfx950: InversePreEmphasis (:84-99, a one-unit
// tanh RNN) and VolNormConv (:7-60, windowed volume normalisation).
//
// InversePreEmphasis:  h[t] = tanh(w_ih x[t] + w_hh h[t-1]),  h[-1] = 0,  per clip.
// The map h -> tanh(a + w_hh h) is a contraction with factor <= |w_hh|, and |h| <= 1: two runs over the same input that start W samples
// back from different states are at most 2 |w_hh|^W apart.  A lane that starts W samples before its chunk with h = 0 therefore reaches its
// chunk with an error <= 2 |w_hh|^W, and W is chosen so that this is <= 2^-25, below half an fp32 ulp of any |h| >= 2^-2 and far below the
// rounding of the fp32 output otherwise (W = 592 at 0.97).  The backward recurrence d[t] = (1 - y[t]^2) (gy[t] + w_hh d[t+1]) is linear with
// the same factor and takes the same scheme mirrored.
//
// Geometry (parallel instance): a workgroup of 256 lanes owns a span of SPAN = 8192 samples of one clip, a lane a chunk of CH = 32.
//   * The chunk length trades warm-up work against lanes: a lane walks W + CH dependent steps, so time ~ (W + CH) * step latency as long as
//     every lane is resident, and the number of lanes is N T / CH.  At the flagship inference shape (16 clips of 10 s, 3.5 M samples) CH = 32
//     gives 110 k lanes = 1723 waves for 1024 SIMDs - everything resident at two waves per SIMD, which also overlaps the chains' latency;
//     CH = 64 would halve the lanes for 5 % fewer steps per lane, CH = 16 doubles the waves (a second round) for 3 % fewer.
//   * The span plus its warm-up is staged through LDS with 16-byte global loads; results go back through LDS and leave with 16-byte
//     stores.  Lanes walk LDS with a stride of one chunk, so the image is pitched: sample i sits at word i + i / 32, i.e. lane l starts
//     at word 33 l + const and the 32 lanes of an LDS access group hit 32 different banks.  No lane walks global memory.
//   * W <= WARM_MAX = 2048 (|w_hh| <= 0.9912) fits the static LDS image (42 KB forward, 84 KB backward).
// Sequential instance: one workgroup per clip, tiles of 8192 samples staged the same way, lane 0 walks.  It covers every |w_hh| whose W
// exceeds WARM_MAX, and |w_hh| >= 1 (and NaN), where the bound does not hold.
// The rule (psnd.h, pytorch_sound_amd.models.sound.ipreemph_warm) is a function of w_hh alone.  The weights are read from DEVICE memory,
// the module's own parameters: nothing is cached on the host, so an in-place edit of any kind counts on the next call.  With
// warm = PSND_IPREEMPH_AUTO the kernel evaluates the rule itself on a grid of the parallel geometry; if it selects the sequential instance,
// workgroup 0 of each clip runs it and the others leave at once.
// The recurrences run in fp64 (inputs and outputs fp32): the chain is latency bound either way, and the result is then the correctly
// rounded trajectory instead of one that drifts from it by 1 / (1 - |w_hh|) times the rounding of every step.
//
// Weight gradients: every lane leaves two double partial sums, a second single-workgroup launch adds them in index order - no atomics,
// bit-reproducible.
//
// VolNormConv: one workgroup per hop; unbiased standard deviation of ALL B * window elements of wav[..., start : start + window] in two
// passes (mean, then squared deviations) accumulated in double, then the hop's own output slice.
#include "psnd_common.h"
#include "psnd_span_stage.h"
#include <math.h>

namespace {

constexpr int LANES = STAGE_LANES;                     // pitched, stage_in, stage_out: psnd_span_stage.h
constexpr int CH = 32;                                  // samples per lane
constexpr int SPAN = PSND_IPREEMPH_SPAN;                // samples per workgroup
constexpr int WARM_MAX = PSND_IPREEMPH_WARM_MAX;
constexpr int IMG = (SPAN + WARM_MAX) / 32 * 33;        // words of one pitched LDS image
static_assert(SPAN == LANES * CH && CH == 32 && WARM_MAX % 32 == 0, "geometry");

// the rule: smallest multiple of 32 with 2 |w_hh|^W <= 2^-25, or PSND_IPREEMPH_SEQ
__device__ __forceinline__ int warm_rule(float w_hh) {
    const double a = fabs((double)w_hh);
    if (!(a < 1.0)) return PSND_IPREEMPH_SEQ;
    if (a < 0x1p-26) return 32;
    const double w = ceil(26.0 * 0.6931471805599453 / -log(a));
    if (!(w <= (double)WARM_MAX)) return PSND_IPREEMPH_SEQ;
    const int W = ((int)w + 31) & ~31;
    return W < 32 ? 32 : W;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
// sum over the workgroup, the same value in every thread; fixed order.  `red` : LANES / 64 doubles of LDS
__device__ __forceinline__ double block_sum_d(double v, double *red) {
    v = wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void ipreemph_fwd_kernel(const float *x, long long T, const float *pw_ih, const float *pw_hh, int warm,
                                                             float *y) {
    __shared__ __attribute__((aligned(16))) float s[IMG];
    const double w_ih = (double)*pw_ih, w_hh = (double)*pw_hh;
    if (warm == PSND_IPREEMPH_AUTO) warm = warm_rule(*pw_hh);
    const float *xr = x + (size_t)blockIdx.y * T;
    float *yr = y + (size_t)blockIdx.y * T;
    if (warm < 0) {                                     // sequential instance: workgroup 0 of the clip, lane 0 walks
        if (blockIdx.x != 0) return;
        double h = 0.0;
        for (long long t0 = 0; t0 < T; t0 += SPAN) {
            const int n = (int)min((long long)SPAN, T - t0), n4 = (n + 3) & ~3;
            stage_in<false>(s, xr, T, t0, n4);
            __syncthreads();
            if (threadIdx.x == 0)
                for (int i = 0; i < n; ++i) {
                    h = tanh(fma(w_hh, h, w_ih * (double)s[i]));
                    s[i] = (float)h;
                }
            __syncthreads();
            stage_out<false>(s, 0, yr, T, t0, n4);
            __syncthreads();
        }
        return;
    }
    const long long b0 = (long long)blockIdx.x * SPAN;  // first sample of the span; staged word i holds sample b0 - warm + i
    const int cover = (int)min((long long)SPAN, (T - b0 + 31) & ~31ll);
    stage_in<true>(s, xr, T, b0 - warm, warm + cover);
    __syncthreads();
    const int l = threadIdx.x;
    float out[CH];
    const bool live = b0 + (long long)l * CH < T;
    if (live) {
        const int ci = warm + l * CH;                   // staged index of the chunk's first sample
        int i = l * CH;                                 // warm-up from here, clamped at the clip start (there h = 0 is exact)
        if (b0 - warm + i < 0) i = (int)(warm - b0);
        double h = 0.0;
        for (; i < ci; ++i) h = tanh(fma(w_hh, h, w_ih * (double)s[pitched(i)]));
        const int p = pitched(ci);
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            h = tanh(fma(w_hh, h, w_ih * (double)s[p + k]));
            out[k] = (float)h;
        }
    }
    __syncthreads();                                    // later lanes have finished reading this chunk as their warm-up
    if (live) {
        const int p = pitched(warm + l * CH);
#pragma unroll
        for (int k = 0; k < CH; ++k) s[p + k] = out[k];
    }
    __syncthreads();
    stage_out<true>(s, warm, yr, T, b0, cover);
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// gx[t] = w_ih d[t];  partial sums of d[t] x[t] and d[t] y[t-1] over the samples this thread stores.  sd : d, sy : y, both images of
// n samples starting at sample t0 (i0 = 0), plain or pitched.
template <bool PITCH>
__device__ __forceinline__ void bwd_out(const float *sd, const float *sy, const float *xr, const float *yr, float *gxr, long long T,
                                        long long t0, int n, double w_ih, double &a_ih, double &a_hh) {
    for (int i = 4 * threadIdx.x; i < n; i += 4 * LANES) {
        const long long t = t0 + i;
        if (t >= T) break;
        const int p = PITCH ? pitched(i) : i;
        f32x4 xv = {0.f, 0.f, 0.f, 0.f}, gv;
        const bool full = t + 3 < T;
        if (full) {
            xv = *reinterpret_cast<const f32x4_u *>(xr + t);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t + k < T) xv[k] = xr[t + k];
        }
        float yp = i > 0 ? sy[PITCH ? pitched(i - 1) : i - 1] : (t > 0 ? yr[t - 1] : 0.f);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double d = (double)sd[p + k];         // zero beyond T
            gv[k] = (float)(w_ih * d);
            a_ih = fma(d, (double)xv[k], a_ih);
            a_hh = fma(d, (double)yp, a_hh);
            yp = sy[p + k];
        }
        if (full) {
            *reinterpret_cast<f32x4_u *>(gxr + t) = gv;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t + k < T) gxr[t + k] = gv[k];
        }
    }
}

__global__ __launch_bounds__(LANES) void ipreemph_bwd_kernel(const float *gy, const float *y, const float *x, long long T, const float *pw_ih,
                                                             const float *pw_hh, int warm, float *gx, double *partial) {
    __shared__ __attribute__((aligned(16))) float sg[IMG];
    __shared__ __attribute__((aligned(16))) float sy[IMG];
    const double w_ih = (double)*pw_ih, w_hh = (double)*pw_hh;
    if (warm == PSND_IPREEMPH_AUTO) warm = warm_rule(*pw_hh);
    const size_t row = (size_t)blockIdx.y * T;
    const float *gyr = gy + row, *yr = y + row, *xr = x + row;
    float *gxr = gx + row;
    double a_ih = 0.0, a_hh = 0.0;
    double *slot = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (2 * LANES) + 2 * threadIdx.x;
    if (warm < 0) {
        if (blockIdx.x == 0) {
            double d = 0.0;
            for (long long t1 = T; t1 > 0; t1 -= SPAN) {    // tiles from the end
                const long long t0 = max(0ll, t1 - SPAN);
                const int n = (int)(t1 - t0), n4 = (n + 3) & ~3;
                stage_in<false>(sg, gyr, t1, t0, n4);       // `t1` as the end: nothing of the later tile
                stage_in<false>(sy, yr, t1, t0, n4);
                __syncthreads();
                if (threadIdx.x == 0)
                    for (int i = n - 1; i >= 0; --i) {
                        const double yv = (double)sy[i];
                        d = fma(-yv, yv, 1.0) * fma(w_hh, d, (double)sg[i]);
                        sg[i] = (float)d;
                    }
                __syncthreads();
                bwd_out<false>(sg, sy, xr, yr, gxr, t1, t0, n4, w_ih, a_ih, a_hh);
                __syncthreads();
            }
        }
        slot[0] = a_ih, slot[1] = a_hh;
        return;
    }
    const long long b0 = (long long)blockIdx.x * SPAN;  // staged word i holds sample b0 + i; the warm-up lies behind the span
    const int cover = (int)min((long long)(SPAN + warm), (T - b0 + 31) & ~31ll);
    stage_in<true>(sg, gyr, T, b0, cover);
    stage_in<true>(sy, yr, T, b0, cover);
    __syncthreads();
    const int l = threadIdx.x;
    float out[CH];
    const bool live = b0 + (long long)l * CH < T;
    if (live) {
        const int ce = (l + 1) * CH;                    // one past the chunk; cover >= ce
        int i = min(ce + warm, cover) - 1;              // beyond T the images hold zeros: d stays exactly 0 there, as d[T] = 0
        double d = 0.0;
        for (; i >= ce; --i) {
            const int p = pitched(i);
            const double yv = (double)sy[p];
            d = fma(-yv, yv, 1.0) * fma(w_hh, d, (double)sg[p]);
        }
        const int p = pitched(l * CH);
#pragma unroll
        for (int k = CH - 1; k >= 0; --k) {
            const double yv = (double)sy[p + k];
            d = fma(-yv, yv, 1.0) * fma(w_hh, d, (double)sg[p + k]);
            out[k] = (float)d;
        }
    }
    __syncthreads();
    if (live) {
        const int p = pitched(l * CH);
#pragma unroll
        for (int k = 0; k < CH; ++k) sg[p + k] = out[k];
    }
    __syncthreads();
    bwd_out<true>(sg, sy, xr, yr, gxr, T, b0, min(cover, SPAN), w_ih, a_ih, a_hh);
    slot[0] = a_ih, slot[1] = a_hh;
}

// gw[0] = sum of partial[2 e], gw[1] = sum of partial[2 e + 1], e < count, in a fixed order
__global__ __launch_bounds__(LANES) void ipreemph_gw_kernel(const double *partial, long long count, float *gw) {
    __shared__ double red[2][LANES];
    double a = 0.0, b = 0.0;
    for (long long e = threadIdx.x; e < count; e += LANES) a += partial[2 * e], b += partial[2 * e + 1];
    red[0][threadIdx.x] = a, red[1][threadIdx.x] = b;
    __syncthreads();
    for (int h = LANES / 2; h >= 1; h >>= 1) {
        if (threadIdx.x < h) red[0][threadIdx.x] += red[0][threadIdx.x + h], red[1][threadIdx.x] += red[1][threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x < 2) gw[threadIdx.x] = (float)red[threadIdx.x][0];
}

// ---- VolNormConv ------------------------------------------------------------------------------------------------------------------
// unbiased standard deviation of wav[b][start + k], b < B, k < window: waves take rows, lanes take samples
__device__ __forceinline__ float window_std(const float *wav, int B, long long L, int window, long long start, double *red) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double n = (double)B * (double)window;
    double s = 0.0;
    for (int b = w; b < B; b += LANES / 64) {
        const float *r = wav + (size_t)b * L + start;
        for (int k = lane; k < window; k += 64) s += (double)r[k];
    }
    const double mean = block_sum_d(s, red) / n;
    double q = 0.0;
    for (int b = w; b < B; b += LANES / 64) {
        const float *r = wav + (size_t)b * L + start;
        for (int k = lane; k < window; k += 64) {
            const double d = (double)r[k] - mean;
            q = fma(d, d, q);
        }
    }
    return (float)sqrt(block_sum_d(q, red) / (n - 1.0));      // one element: 0 / 0, NaN as torch.std
}

// REVERSE: out = wav * (std[i] / gain) with std given;  else std[i] computed and written, out = wav / (std[i] * gain) (gain = 1 / 10^(db/10))
template <bool REVERSE>
__global__ __launch_bounds__(LANES) void volnorm_kernel(const float *wav, int B, long long L, int window, int hop, float gain, float *out,
                                                        long long out_len, float *stdv) {
    __shared__ double red[LANES / 64];
    const long long start = (long long)blockIdx.x * hop;
    const long long stop = blockIdx.x + 1 == gridDim.x ? out_len : start + hop;     // the last hop carries the tail rule (host: out_len)
    float scale;
    if (REVERSE) {
        scale = stdv[blockIdx.x] / gain;
    } else {
        const float sd = window_std(wav, B, L, window, start, red);
        if (threadIdx.x == 0) stdv[blockIdx.x] = sd;
        scale = sd * gain;
    }
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = w; b < B; b += LANES / 64) {
        const float *r = wav + (size_t)b * L;
        float *o = out + (size_t)b * out_len;
        for (long long t = start + lane; t < stop; t += 64) o[t] = REVERSE ? r[t] * scale : r[t] / scale;
    }
}

// hops of the loops `for start in range(0, L - window, hop)`; 0 when there is none
inline long long volnorm_hops(long long L, int window, int hop) { return L > window ? (L - window + hop - 1) / hop : 0; }

int volnorm_check(const char *what, const void *wav, const void *out, const void *stdv, int64_t B, int64_t L, int window, int hop, float gain,
                  int64_t out_len, long long *hops) {
    if (!wav || !out || !stdv) PSND_FAIL(PSND_E_ARG, "%s: null pointer", what);
    if (window < 1 || hop < 1 || !(gain > 0.f)) PSND_FAIL(PSND_E_ARG, "%s: window=%d hop=%d gain=%g", what, window, hop, (double)gain);
    if (B < 1 || B > 0x7fffffff || L <= window) PSND_FAIL(PSND_E_SHAPE, "%s: B=%lld L=%lld window=%d", what, (long long)B, (long long)L, window);
    const long long n = volnorm_hops(L, window, hop);
    if (n > 0x7fffffff) PSND_FAIL(PSND_E_SHAPE, "%s: %lld hops", what, n);
    if (out_len <= (n - 1) * hop || out_len > L)        // the last hop's slice [(n - 1) hop, out_len) is non-empty and inside the signal
        PSND_FAIL(PSND_E_SHAPE, "%s: out_len=%lld for L=%lld window=%d hop=%d", what, (long long)out_len, (long long)L, window, hop);
    *hops = n;
    return PSND_OK;
}

int ipreemph_check(const char *what, int64_t N, int64_t T, int warm) {
    if (N < 0 || N > 65535 || T < 0) PSND_FAIL(PSND_E_SHAPE, "%s: N=%lld T=%lld", what, (long long)N, (long long)T);
    if (warm != PSND_IPREEMPH_AUTO && warm != PSND_IPREEMPH_SEQ && (warm < 32 || warm > WARM_MAX || warm % 32))
        PSND_FAIL(PSND_E_ARG, "%s: warm=%d (a multiple of 32 in [32, %d], PSND_IPREEMPH_SEQ or PSND_IPREEMPH_AUTO)", what, warm, WARM_MAX);
    if ((T + SPAN - 1) / SPAN > 0x7fffffff) PSND_FAIL(PSND_E_SHAPE, "%s: T=%lld", what, (long long)T);
    return PSND_OK;
}

}  // namespace

extern "C" int psnd_ipreemph_fwd(const float *x, int64_t N, int64_t T, const float *w_ih, const float *w_hh, int warm, float *y, void *stream) {
    if (!x || !y || !w_ih || !w_hh) PSND_FAIL(PSND_E_ARG, "ipreemph_fwd: null pointer");
    if (int rc = ipreemph_check("ipreemph_fwd", N, T, warm)) return rc;
    if (N == 0 || T == 0) return PSND_OK;
    const unsigned gx = warm == PSND_IPREEMPH_SEQ ? 1u : (unsigned)((T + SPAN - 1) / SPAN);
    hipLaunchKernelGGL(ipreemph_fwd_kernel, dim3(gx, (unsigned)N), dim3(LANES), 0, static_cast<hipStream_t>(stream), x, (long long)T, w_ih, w_hh,
                       warm, y);
    PSND_CHECK_LAUNCH("ipreemph_fwd");
    return PSND_OK;
}

extern "C" int psnd_ipreemph_bwd(const float *gy, const float *y, const float *x, int64_t N, int64_t T, const float *w_ih, const float *w_hh,
                                 int warm, float *gx, double *partial, float *gw, void *stream) {
    if (!gy || !y || !x || !gx || !partial || !gw || !w_ih || !w_hh) PSND_FAIL(PSND_E_ARG, "ipreemph_bwd: null pointer");
    if (int rc = ipreemph_check("ipreemph_bwd", N, T, warm)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    long long count = 0;
    if (N > 0 && T > 0) {
        const unsigned gxn = warm == PSND_IPREEMPH_SEQ ? 1u : (unsigned)((T + SPAN - 1) / SPAN);
        hipLaunchKernelGGL(ipreemph_bwd_kernel, dim3(gxn, (unsigned)N), dim3(LANES), 0, st, gy, y, x, (long long)T, w_ih, w_hh, warm, gx, partial);
        PSND_CHECK_LAUNCH("ipreemph_bwd");
        count = (long long)gxn * N * LANES;
    }
    hipLaunchKernelGGL(ipreemph_gw_kernel, dim3(1), dim3(LANES), 0, st, (const double *)partial, count, gw);
    PSND_CHECK_LAUNCH("ipreemph_bwd (weight gradients)");
    return PSND_OK;
}

extern "C" int psnd_volnorm_fwd(const float *wav, int64_t B, int64_t L, int window, int hop, float inv_gain, float *out, int64_t out_len,
                                float *std, void *stream) {
    long long hops;
    if (int rc = volnorm_check("volnorm_fwd", wav, out, std, B, L, window, hop, inv_gain, out_len, &hops)) return rc;
    hipLaunchKernelGGL(volnorm_kernel<false>, dim3((unsigned)hops), dim3(LANES), 0, static_cast<hipStream_t>(stream), wav, (int)B, (long long)L,
                       window, hop, inv_gain, out, (long long)out_len, std);
    PSND_CHECK_LAUNCH("volnorm_fwd");
    return PSND_OK;
}

extern "C" int psnd_volnorm_reverse(const float *wav, int64_t B, int64_t L, int window, int hop, float gain, const float *std, float *out,
                                    int64_t out_len, void *stream) {
    long long hops;
    if (int rc = volnorm_check("volnorm_reverse", wav, out, std, B, L, window, hop, gain, out_len, &hops)) return rc;
    hipLaunchKernelGGL(volnorm_kernel<true>, dim3((unsigned)hops), dim3(LANES), 0, static_cast<hipStream_t>(stream), wav, (int)B, (long long)L,
                       window, hop, gain, out, (long long)out_len, const_cast<float *>(std));
    PSND_CHECK_LAUNCH("volnorm_reverse");
    return PSND_OK;
}
