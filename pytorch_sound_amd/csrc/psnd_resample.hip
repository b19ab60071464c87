// psnd_resample.hip - sample-rate conversion by a rational factor up / down per row of an (N, T) fp32 tensor on gfx950, and its adjoint.
// The reference shells out for this (scripts/preprocess.py:82-88 sox `rate`, :32-41 ffmpeg); the definition here is the one of
// scipy.signal.resample_poly with zero padding (include/psnd.h):
//
//   y[m] = sum_i x[i] g[m down - i up + P],   P = (taps - 1) / 2,   over 0 <= i < T with 0 <= m down - i up + P <= 2P
//
// With c = m down + P the inputs that meet output m are i = floor(c / up) - j, j = 0, 1, ..., and their taps g[phi + j up],
// phi = c mod up: one phase of the filter, at most K = ceil(taps / up) products.  Outputs m and m + up share a phase.
// The adjoint (the input gradient) is the same sum with up and down exchanged and g reversed, so `flip` is all it takes: g is reversed
// while it is loaded, and the kernel has one instance.
//
// Geometry.  A workgroup of 256 lanes owns TILE = 1024 consecutive outputs of one row, lane t the outputs t, t + 256, ... of the tile
// (coalesced stores).  LDS holds
//   g    all `taps` values in natural order.  A contiguous tile meets every phase, so it needs them all; they come from L2 once per
//        workgroup (8821 values per 1024 outputs at 320 / 441 - a third of the 28 LDS reads per output that follow).  At a fixed j lanes
//        t and t + 1 read words (down mod up) apart (modulo the wrap at up): an odd distance for every pair of usual audio rates but
//        441 / 320, where the wrap (441 is odd) still spreads a 32-lane group over the banks two lanes deep; up <= 3 reads at most three
//        neighbouring words (broadcast).
//   xs   the span of x that the tile reaches, i in [ceil((c_first - 2P) / up), floor(c_last / up)], in pieces of XS = 3072 samples, plain
//        order.  One piece covers a tile while 1024 down / up + K <= 3072: it is staged with zeros where it leaves the row, every output
//        then has floor(taps / up) products or one more whatever its place in the row, and the four outputs of a lane advance through
//        one loop with one trip count (eight independent LDS reads per step; a pure decimation, up = 1, has one phase, and the four
//        outputs share each tap: five).  A steeper decimation takes several pieces, each between two barriers, and every output adds
//        the products whose x falls into the piece at hand.
//        Lanes step through x by down / up words: at down / up = 2 lanes l and l + 16 of a 32-lane group meet on a bank (ds_read_b32,
//        32 banks).  A pitched image (word q at q + q / 32) removes that conflict at a shift and an add per read; the plain image
//        with a deeper unroll measured a quarter faster than the pitched one (profiles/NOTEBOOK.md), so the conflict stays.
// g and xs together stay under 64 KB (12801 + 3072 words): PSND_RESAMPLE_MAX_TAPS.  The LDS is sized per launch to the taps at hand.
// Accumulation is fp32 by fma, from the newest sample to the oldest; no atomics, fixed order: the same bits every run.  A zero staged
// beyond the row meets a finite tap and adds nothing; samples inside the row meet exactly the taps of the definition, so a NaN reaches the
// outputs whose window covers it and no others.
#include "psnd_common.h"

namespace {

constexpr int LANES = 256;
constexpr int TILE = PSND_RESAMPLE_TILE;
constexpr int R = TILE / LANES;                         // outputs per lane
constexpr int XS = 3072;                                // samples of x per staged piece
static_assert(TILE % LANES == 0 && XS % 32 == 0, "geometry");
static_assert((PSND_RESAMPLE_MAX_TAPS + 3 + XS) * 4 <= 65536, "g and the x image share 64 KB of LDS");

__host__ __device__ inline int g_words(int taps) { return (taps + 3) & ~3; }

__global__ __launch_bounds__(LANES) void resample_kernel(const float *__restrict__ x, long long T, const float *__restrict__ h, int taps,
                                                         int up, int down, int flip, float *__restrict__ y, long long T_out, int tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *g = lds;
    float *xs = lds + g_words(taps);
    const int tid = threadIdx.x;
    const long long row = blockIdx.x / tiles;
    const long long m0 = (long long)(blockIdx.x % tiles) * TILE;
    const int nout = (int)min((long long)TILE, T_out - m0);
    const float *xr = x + (size_t)row * T;
    for (int k = tid; k < taps; k += LANES) g[k] = h[flip ? taps - 1 - k : k];

    const int P = taps >> 1;
    const long long c0 = m0 * down + P;                                 // c of the tile's first and last output
    const long long c1 = (m0 + nout - 1) * down + P;
    const long long lo = c0 - (taps - 1);
    const long long s_lo = lo >= 0 ? (lo + up - 1) / up : -((-lo) / up);  // ceil(lo / up): the oldest and the newest sample the tile reaches,
    const long long s_hi = c1 / up;                                     // before the row's ends cut them

    int phi[R], top[R], jmax[R];
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const long long c = c0 + (long long)(tid + r * LANES) * down;
        const long long ih = c / up;
        phi[r] = (int)(c - ih * up);
        top[r] = (int)(ih - s_lo);                                      // the newest sample of this output, relative to s_lo
        jmax[r] = phi[r] < taps ? (taps - 1 - phi[r]) / up : -1;        // fewer taps than phases: this phase may have none
        acc[r] = 0.f;
    }
    if (s_hi - s_lo < XS) {
        // one piece holds the whole span, zeros where it leaves the row: every phase has kmin = floor(taps / up) products or one more, so
        // the loop has one trip count for all lanes and all R outputs of a lane advance together - 2 R independent LDS reads per step
        const int n = (int)(s_hi - s_lo + 1);
        for (int q = tid; q < n; q += LANES) {
            const long long i = s_lo + q;
            xs[q] = i >= 0 && i < T ? xr[i] : 0.f;
        }
        __syncthreads();
        const int kmin = taps / up;
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (tid + r * LANES >= nout) top[r] = kmin - 1, phi[r] = 0, jmax[r] = -1;      // no output: reads that stay inside, no tail
        if (up == 1) {                                                  // one phase: the outputs of a lane share the tap
#pragma unroll 4
            for (int j = 0; j < kmin; ++j) {
                const float gj = g[j];
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(xs[top[r] - j], gj, acc[r]);
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < kmin; ++j) {
#pragma unroll
                for (int r = 0; r < R; ++r) acc[r] = __builtin_fmaf(xs[top[r] - j], g[phi[r] + j * up], acc[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (jmax[r] >= kmin) acc[r] = __builtin_fmaf(xs[top[r] - kmin], g[phi[r] + kmin * up], acc[r]);
    } else {
        // a steep decimation: the span in pieces, every output adds the products whose sample lies in the piece at hand
        const long long i_lo = max(s_lo, 0ll), i_hi = min(s_hi, T - 1);
        const int shift = (int)(i_lo - s_lo);
        for (long long base = i_lo; base <= i_hi; base += XS) {
            const int n = (int)min((long long)XS, i_hi - base + 1);
            __syncthreads();                                            // g is written; the piece before this one is used up
            for (int q = tid; q < n; q += LANES) xs[q] = xr[base + q];
            __syncthreads();
            const int b = (int)(base - i_lo);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (tid + r * LANES >= nout) continue;
                // sample t - j lies in the piece [b, b + n), t = the newest sample relative to i_lo
                const int t = top[r] - shift;
                const int jlo = max(0, t - (b + n - 1)), jhi = min(jmax[r], t - b);
                const float *gp = g + phi[r];
                const int q0 = t - b;
                float a = acc[r];
                for (int j = jlo; j <= jhi; ++j) a = __builtin_fmaf(xs[q0 - j], gp[j * up], a);
                acc[r] = a;
            }
        }
    }
    float *yr = y + (size_t)row * T_out + m0;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (tid + r * LANES < nout) yr[tid + r * LANES] = acc[r];
}

}  // namespace

extern "C" int64_t psnd_resample_len(int64_t T, int up, int down) {
    if (T <= 0 || up <= 0 || down <= 0) return 0;
    return (int64_t)(((__int128)T * up + down - 1) / down);
}

extern "C" int psnd_resample(const float *x, int64_t N, int64_t T, const float *h, int taps, int up, int down, int flip, float *y,
                             int64_t T_out, void *stream) {
    if (taps <= 0 || taps % 2 == 0) PSND_FAIL(PSND_E_ARG, "resample: taps=%d (an odd, positive count: 2P + 1)", taps);
    if (taps > PSND_RESAMPLE_MAX_TAPS)
        PSND_FAIL(PSND_E_ARG, "resample: taps=%d is more than PSND_RESAMPLE_MAX_TAPS=%d", taps, PSND_RESAMPLE_MAX_TAPS);
    if (up <= 0 || down <= 0) PSND_FAIL(PSND_E_ARG, "resample: up=%d down=%d", up, down);
    if (N < 0 || T < 0 || T_out < 0) PSND_FAIL(PSND_E_ARG, "resample: N=%lld T=%lld T_out=%lld", (long long)N, (long long)T, (long long)T_out);
    if (flip != 0 && flip != 1) PSND_FAIL(PSND_E_ARG, "resample: flip=%d", flip);
    if (x && (const void *)x == (const void *)y) PSND_FAIL(PSND_E_ARG, "resample: x and y must be different buffers");
    if (N == 0 || T_out == 0) return PSND_OK;
    if (!y || !h || (!x && T > 0)) PSND_FAIL(PSND_E_ARG, "resample: null pointer");
    const long long tiles = (T_out + TILE - 1) / TILE;
    if (N > 0x7fffffff || tiles > 0x7fffffff || N * tiles > 0x7fffffff)
        PSND_FAIL(PSND_E_SHAPE, "resample: N=%lld T_out=%lld is more than 2^31 - 1 workgroups", (long long)N, (long long)T_out);
    const size_t lds = (size_t)(g_words(taps) + XS) * sizeof(float);
    hipLaunchKernelGGL(resample_kernel, dim3((unsigned)(N * tiles)), dim3(LANES), lds, static_cast<hipStream_t>(stream), x, (long long)T, h,
                       taps, up, down, flip, y, (long long)T_out, (int)tiles);
    PSND_CHECK_LAUNCH("resample");
    return PSND_OK;
}
