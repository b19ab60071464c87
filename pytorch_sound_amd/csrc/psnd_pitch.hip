// psnd_pitch.hip - fundamental frequency per frame of an (N, T) fp32 tensor on gfx950: YIN (de Cheveigne & Kawahara 2002, steps 1-5) by the
// definition of include/psnd.h.  It stands where the reference's utils/sound.py get_f0 (:38-49) calls WORLD through pyworld; it is not WORLD.
//
// The cost is the difference function: W tau_max subtract-square-add pairs per frame (193 k at 22.05 kHz with the defaults), each frame on
// its own - no partial sum is shared between overlapping frames, which would change the conditioning of d.
//
// One launch.  A workgroup of WAVES = 4 waves owns WAVES consecutive frames of one row and stages their samples in LDS once: the union of
// the spans when hop < span (sample g0 + p at word p), the spans back to back otherwise (frames then share nothing, and a union would grow
// with hop).  Samples outside [0, len_row) are staged as zeros - no global read leaves the row's valid part - and 64 words behind the last
// span are staged the same way, so that the lanes of the last lag group, which own lags beyond tau_max, read inside the array.
//   wave = frame, lane l = the lags 1 + l + 64 k.  u[j + tau] is consecutive across the lanes: one conflict-free ds_read_b32 per pair.  u[j]
//   is no LDS read at all: a lane loads u[jb + l] once per 64 values of j and v_readlane hands value jj to the whole wave in a scalar
//   register, which the subtract takes as an operand.  Up to KC_MAX = 5 lag groups (320 lags) are carried in registers per pass over j.
//   d goes to the wave's own row of LDS; the prefix sum of step 2 is a shuffle scan per group of 64 lags with a carried total, d' replaces d
//   in place, "first lag under the threshold" is a ballot, the descent and the parabola are a short uniform walk over d' in LDS.
// Nothing is exchanged between waves behind the one barrier after staging, so waves whose frame lies behind the row's count or holds a
// non-finite sample write (0, 1, 0) and leave.
#include "psnd_common.h"

namespace {

constexpr int WAVES = 4;
constexpr int LANES = 64 * WAVES;
constexpr int KC_MAX = 5;
constexpr int PAD = 64;
constexpr int MAX_SPAN = 6144;                          // 4 (4 span + PAD + 4 (tau_max + 64)) bytes <= 150 KiB for every W >= tau_max

__device__ __forceinline__ long long row_len(const long long *lengths, long long row, long long T) {
    if (!lengths) return T;
    const long long v = lengths[row];
    return v < 0 ? 0 : (v > T ? T : v);
}

// LDS words written by some lanes of a wave and read by others of the SAME wave: its LDS operations complete in order, the clobber keeps
// the compiler from moving a read in front of a write
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// d(tau) for the lags tau = 1 + 64 (g0 + k) + lane, k < KC, of the frame whose span starts at u: j ascending, fp32
template <int KC>
__device__ __forceinline__ void diff_pass(const float *u, int W, int g0, int lane, float *d) {
    float acc[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) acc[k] = 0.f;
    const float *ul = u + 1 + 64 * g0 + lane;           // u[j + tau_k] = ul[j + 64 k]
    for (int jb = 0; jb < W; jb += 64) {
        const int held = __float_as_int(u[jb + lane]);  // jb + lane < W + 63: inside the padded array
        const int n = min(64, W - jb);
        const float *uj = ul + jb;
        if (n == 64) {
#pragma unroll 16
            for (int jj = 0; jj < 64; ++jj) {
                const float a = __int_as_float(__builtin_amdgcn_readlane(held, jj));
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const float t = a - uj[jj + 64 * k];
                    acc[k] = __builtin_fmaf(t, t, acc[k]);
                }
            }
        } else {
            for (int jj = 0; jj < n; ++jj) {
                const float a = __int_as_float(__builtin_amdgcn_readlane(held, jj));
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const float t = a - uj[jj + 64 * k];
                    acc[k] = __builtin_fmaf(t, t, acc[k]);
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KC; ++k) d[1 + 64 * (g0 + k) + lane] = acc[k];
}

__global__ __launch_bounds__(LANES) void yin_kernel(const float *__restrict__ x, long long T, const long long *__restrict__ lengths,
                                                    long long hop, int W, int tau_min, int tau_max, float thr, double sr,
                                                    float *__restrict__ f0, float *__restrict__ ap, int *__restrict__ lag, long long F,
                                                    long long groups) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int span = W + tau_max, H = span / 2;
    const int ng = (tau_max + 63) >> 6;                 // groups of 64 lags
    const long long row = blockIdx.x / groups;
    const long long fbase = (long long)(blockIdx.x % groups) * WAVES;
    const long long len = row_len(lengths, row, T);
    const long long nfr = len / hop + 1;                // frames of this row; the slots [nfr, F) are filled
    const long long f = fbase + w;
    const size_t o = (size_t)row * F + f;
    const bool overlap = hop < span;
    const int fs = overlap ? (int)hop : span;           // LDS words between the spans of neighbouring frames
    const int nS = (WAVES - 1) * fs + span + PAD;
    float *S = smem;
    float *D = smem + nS + w * (64 * ng + 1);           // this wave's d / d', indexed by the lag
    if (fbase < nfr) {                                  // the whole workgroup or none of it: a group behind the row's frames stages nothing
        const float *xr = x + (size_t)row * T;
        for (int p = tid; p < nS; p += LANES) {
            long long g;
            if (overlap) {
                g = fbase * hop - H + p;
            } else {
                const int wf = min(p / span, WAVES - 1);
                g = (fbase + wf) * hop - H + (p - wf * span);
            }
            S[p] = (g >= 0 && g < len) ? xr[g] : 0.f;
        }
    }
    __syncthreads();
    if (f >= F) return;
    if (f >= nfr) {
        if (lane == 0) f0[o] = 0.f, ap[o] = 1.f, lag[o] = 0;
        return;
    }
    const float *u = S + w * fs;
    // 6: a non-finite sample anywhere in the span, by its exponent bits
    bool bad = false;
    for (int j = lane; j < span; j += 64) bad |= (__float_as_uint(u[j]) & 0x7f800000u) == 0x7f800000u;
    if (__ballot(bad)) {
        if (lane == 0) f0[o] = 0.f, ap[o] = 1.f, lag[o] = 0;
        return;
    }
    // 1: the difference function
    for (int g0 = 0; g0 < ng; g0 += KC_MAX) {
        switch (min(KC_MAX, ng - g0)) {
            case 1: diff_pass<1>(u, W, g0, lane, D); break;
            case 2: diff_pass<2>(u, W, g0, lane, D); break;
            case 3: diff_pass<3>(u, W, g0, lane, D); break;
            case 4: diff_pass<4>(u, W, g0, lane, D); break;
            default: diff_pass<5>(u, W, g0, lane, D); break;
        }
    }
    // 2, 3: cumulative-mean normalisation in place, the first lag under the threshold, the smallest d' of the search range
    float carry = 0.f, best = __int_as_float(0x7f800000);
    int t0 = 0;
    for (int g = 0; g < ng; ++g) {
        const int tau = 1 + 64 * g + lane;
        const float dv = tau <= tau_max ? D[tau] : 0.f; // a lane reads what it wrote; lags beyond tau_max are left out of the sum
        float s = dv;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const float up = __shfl_up(s, k, 64);
            if (lane >= k) s += up;
        }
        s += carry;
        carry = __shfl(s, 63, 64);
        const float dp = s == 0.f ? 1.f : dv * (float)tau / s;
        const bool in = tau >= tau_min && tau <= tau_max;
        if (tau <= tau_max) D[tau] = dp;
        if (in) best = fminf(best, dp);
        const unsigned long long under = __ballot(in && dp < thr);
        if (t0 == 0 && under) t0 = 1 + 64 * g + __builtin_ctzll(under);
    }
    wave_lds_sync();
    if (t0 == 0) {
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) best = fminf(best, __shfl_xor(best, k, 64));
        if (lane == 0) f0[o] = 0.f, ap[o] = best, lag[o] = 0;
        return;
    }
    // 4, 5: down to the local minimum, then the parabola through its neighbours (every lane walks the same lags: broadcast reads)
    int t = t0;
    float cur = D[t];
    while (t + 1 <= tau_max) {
        const float nx = D[t + 1];
        if (!(nx < cur)) break;
        cur = nx;
        ++t;
    }
    float off = 0.f;
    if (t - 1 >= 1 && t + 1 <= tau_max) {
        const float y0 = D[t - 1], y2 = D[t + 1];
        const float den = y0 - 2.f * cur + y2;
        if (den > 0.f) off = fminf(fmaxf(0.5f * (y0 - y2) / den, -0.5f), 0.5f);
    }
    if (lane == 0) {
        f0[o] = (float)(sr / ((double)t + (double)off));
        ap[o] = cur;
        lag[o] = t;
    }
}

}  // namespace

extern "C" int64_t psnd_yin_frames(int64_t T, int64_t hop) { return (T < 0 || hop < 1) ? 0 : T / hop + 1; }

extern "C" int64_t psnd_yin_max_span(void) { return MAX_SPAN; }

extern "C" int psnd_yin_f0(const float *x, int64_t N, int64_t T, const int64_t *lengths, int64_t hop, int64_t W, int64_t tau_min,
                           int64_t tau_max, float threshold, double sr, float *f0, float *aperiodicity, int32_t *lag, int64_t F,
                           void *stream) {
    if (hop < 1) PSND_FAIL(PSND_E_ARG, "yin: hop=%lld (at least one sample)", (long long)hop);
    if (tau_min < 2 || tau_max < tau_min || W < tau_max)
        PSND_FAIL(PSND_E_ARG, "yin: tau_min=%lld tau_max=%lld W=%lld (2 <= tau_min <= tau_max <= W)", (long long)tau_min, (long long)tau_max,
                  (long long)W);
    if (W > MAX_SPAN || W + tau_max > MAX_SPAN)
        PSND_FAIL(PSND_E_ARG, "yin: span = W + tau_max = %lld + %lld, the kernel stages at most psnd_yin_max_span() = %d samples per frame",
                  (long long)W, (long long)tau_max, MAX_SPAN);
    if (!(threshold > 0.f) || !(sr > 0.0)) PSND_FAIL(PSND_E_ARG, "yin: threshold=%g sr=%g (both positive)", (double)threshold, sr);
    if (N < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "yin: N=%lld T=%lld", (long long)N, (long long)T);
    if (F < psnd_yin_frames(T, hop))
        PSND_FAIL(PSND_E_ARG, "yin: F=%lld, a row of T=%lld with hop=%lld has psnd_yin_frames = %lld frames", (long long)F, (long long)T,
                  (long long)hop, (long long)psnd_yin_frames(T, hop));
    if (N == 0) return PSND_OK;
    if ((!x && T > 0) || !f0 || !aperiodicity || !lag) PSND_FAIL(PSND_E_ARG, "yin: null pointer");
    if (hop > T) hop = T + 1;                           // one frame per row for every hop beyond the row: keeps frame * hop small
    const long long groups = (F + WAVES - 1) / WAVES;
    if (groups > 0x7fffffff || N > 0x7fffffff || N * groups > 0x7fffffff)
        PSND_FAIL(PSND_E_SHAPE, "yin: N=%lld F=%lld is more than 2^31 - 1 workgroups", (long long)N, (long long)F);
    const int span = (int)(W + tau_max), ng = (int)((tau_max + 63) / 64);
    const int fs = hop < span ? (int)hop : span;
    const size_t lds = sizeof(float) * ((size_t)(WAVES - 1) * fs + span + PAD + (size_t)WAVES * (64 * ng + 1));
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(yin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) PSND_FAIL(PSND_E_HIP, "yin: set LDS size: %s", hipGetErrorString(e));
    }
    hipLaunchKernelGGL(yin_kernel, dim3((unsigned)(N * groups)), dim3(LANES), lds, static_cast<hipStream_t>(stream), x, (long long)T,
                       reinterpret_cast<const long long *>(lengths), (long long)hop, (int)W, (int)tau_min, (int)tau_max, threshold, sr, f0,
                       aperiodicity, reinterpret_cast<int *>(lag), (long long)F, groups);
    PSND_CHECK_LAUNCH("yin");
    return PSND_OK;
}
