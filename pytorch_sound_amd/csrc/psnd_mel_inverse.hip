// psnd_mel_inverse.hip - mel to linear magnitude on (N, M, F) fp32 mels on gfx950, by the definition of include/psnd.h: per frame the
// non-negative least-squares problem min_{x >= 0} |A x - b|^2, A the row-normalised filterbank, solved by n_iter steps of FISTA from the
// flat-band guess.  What kernels.mel_inverse, InverseMelScale and mel_to_wave are built on.
//
// One launch for the whole loop.  A workgroup of 256 lanes owns T = psnd_mel_inverse_tile(M, K) consecutive frames of one item (the
// fastest axis: loads of Y and stores of x are runs of T floats).  The iterates x and z (K x T each), the residual r and the right-hand
// side b (M x T each) live in LDS from the first iteration to the last: T (2 K + 2 M) floats.  Y is read once, x written once, nothing
// goes to global memory in between; no scratch, no atomics.  An iteration is two passes with a barrier behind each:
//     r[m] = sum_{k in band(m)} A[m, k] z[k] - b[m]                                         (M T sums)
//     g = sum_{m in band(k)} A[m, k] r[m];  x' = max(z - step g, 0);  z = x' + beta (x' - x)  (K T sums)
// Only the band of a row or a column is walked - from its first to its last non-zero weight; the plan holds both as packed runs with
// their {first, length, offset} - so a mel filterbank costs its ~2 weights per bin, not M.  Plain vector FMAs: the fp32 MFMA has the
// vector rate on this part, and its 16 x 4 granularity would multiply mostly the zeros of a band two to three filters wide.
//   A lane works on FR = 4 consecutive frames of the tile (2 where T = 2) and on the rows l / (T / FR), + 256 FR / T, ... of whatever is
//   being formed: a weight is read once for its FR frames, their values come and go as one 16-byte LDS access, and the FR chains of
//   multiply-adds are independent.  The launch is bound by the latency of dependent LDS reads (band, weights, values, sum), not by
//   arithmetic; the stages that led here are timed in profiles/NOTEBOOK.md.
//   The band tables and the packed weights are one run of the plan (12.7 KB at 80 x 513).  Where the run fits TAB_WORDS of LDS behind
//   the state arrays a workgroup copies it there once and reads it from LDS; a larger run (128 x 2049, a dense matrix) is read from
//   global memory, the band of a lane's next row asked for ahead of time.  The host cannot see the length of the run (the plan lives on
//   the device): it asks for the LDS whenever the band tables alone (2 M + 2 K words) fit, and a plan whose weights then do not fit
//   leaves that LDS unused.
//   Every sum runs in ascending index order with one fused multiply-add per term and a lane's frames share nothing: a frame's bits depend
//   on its own column of Y alone, wherever it lies and whichever road the tables take.
//   A plan that is not one (magic), that was built for another (M, K) or for fewer iterations cannot be refused by the host either: such
//   a launch reads nothing but the plan's header and fills out and resid with NaN.
#include "psnd_common.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int THREADS = 256;
constexpr int MAX_M = 256;
constexpr int MAX_K = 2049;
constexpr int MAX_ITER = 4096;
constexpr int MAX_TILE = 16;
constexpr int LDS_WORDS = 16384;               // 64 KB: what a workgroup may take without asking the runtime for more
constexpr int TAB_WORDS = 4000;                // LDS for the band tables and weights when they fit: 3 workgroups per CU at 80 x 513
constexpr unsigned MAGIC = 0x4D494E56u;        // 'MINV'
constexpr int HDR = 32;

// the plan, in 4-byte words (include/psnd.h)
enum { H_MAGIC, H_M, H_K, H_NMAX, H_NNZR, H_NNZC, H_STEP, H_ZERO, H_D, H_CINV, H_BETA, H_RBAND, H_CBAND, H_RVALS, H_CVALS, H_A, H_F64,
       H_WORDS };

struct Layout {
    int f64, d, cinv, beta, rband, cband, A, vals, words;
};

Layout layout(int M, int K) {
    Layout l;
    l.f64 = HDR;
    l.d = l.f64 + 2 * (2 + M + K);
    l.cinv = l.d + M;
    l.beta = l.cinv + K;
    l.A = l.beta + MAX_ITER;
    l.rband = l.A + M * K;                      // from here on one run: row bands, column bands, row weights, column weights
    l.cband = l.rband + 2 * M;
    l.vals = l.cband + 2 * K;
    l.words = l.vals + 2 * M * K;
    return l;
}

int tile_of(int M, int K) {
    if (M <= 0 || K <= 0 || M > MAX_M || K > MAX_K) return 0;
    int T = MAX_TILE;
    while (T > 1 && T * (2 * K + 2 * M) > LDS_WORDS) T >>= 1;
    return T;
}

struct MiParams {
    const float *Y;
    const unsigned *plan;
    const long long *frames;
    float *out, *resid;
    unsigned F, tiles;
    int M, K, T, n_iter, log_kind, tab_cap;
    float log_offset;
};

__device__ __forceinline__ float undo_log(float y, int kind, float off) {
    if (kind == PSND_LOG_E) return expf(y) - off;
    if (kind == PSND_LOG_10) return exp10f(y) - off;
    return y;
}

typedef unsigned u32x2_u __attribute__((ext_vector_type(2), aligned(4)));       // the band tables start on any word of the plan

// the {first | length << 16, offset} of row (or column) i; (0, 0) past the end - a lane asks for its next row ahead of time
__device__ __forceinline__ u32x2 band_of(const unsigned *__restrict__ band, int i, int n) {
    if (i >= n) return u32x2{0u, 0u};
    const u32x2_u h = *reinterpret_cast<const u32x2_u *>(band + 2 * i);
    return u32x2{h.x, h.y};
}

// FR consecutive frames of one row of an LDS array: one 8- or 16-byte access (the arrays and T FR-float aligned)
template <int FR>
struct Frames {
    float v[FR];
};
template <int FR>
__device__ __forceinline__ Frames<FR> lds_get(const float *q) {
    Frames<FR> o;
    if constexpr (FR == 4) {
        const f32x4 w = *reinterpret_cast<const f32x4 *>(q);
        o.v[0] = w.x, o.v[1] = w.y, o.v[2] = w.z, o.v[3] = w.w;
    } else {
        const f32x2 w = *reinterpret_cast<const f32x2 *>(q);
        o.v[0] = w.x, o.v[1] = w.y;
    }
    return o;
}
template <int FR>
__device__ __forceinline__ void lds_put(float *q, const Frames<FR> &o) {
    if constexpr (FR == 4)
        *reinterpret_cast<f32x4 *>(q) = f32x4{o.v[0], o.v[1], o.v[2], o.v[3]};
    else
        *reinterpret_cast<f32x2 *>(q) = f32x2{o.v[0], o.v[1]};
}

// sums over the band h of one row (or column) for FR frames at once: acc[e] += vals[off + j] v[(lo + j) T + t0 + e], j ascending - every
// frame its own chain of fused multiply-adds, the weight read once for all of them
template <int FR>
__device__ __forceinline__ Frames<FR> band_dot(u32x2 h, const float *__restrict__ vals, const float *v, int T, int t0) {
    const unsigned a = h.x, off = h.y;
    const int lo = a & 0xffff, len = a >> 16;
    const float *w = vals + off;
    const float *q = v + lo * T + t0;
    Frames<FR> acc;
#pragma unroll
    for (int e = 0; e < FR; ++e) acc.v[e] = 0.f;
    for (int j = 0; j < len; ++j) {
        const float wj = w[j];
        const Frames<FR> u = lds_get<FR>(q + j * T);
#pragma unroll
        for (int e = 0; e < FR; ++e) acc.v[e] = __builtin_fmaf(wj, u.v[e], acc.v[e]);
    }
    return acc;
}

// TAB: the band tables and the packed weights (one run of the plan) were copied to LDS behind the state arrays and are read from there.
// FR: the consecutive frames a lane works on (4, or 2 where the tile has only 2): lane l the frames FR (l % (T / FR)) .. and the rows
// l / (T / FR), + 256 FR / T, ...
template <bool TAB, int FR>
__device__ __forceinline__ void mel_inverse_body(const MiParams &p, float *smem) {
    const int T = p.T, M = p.M, K = p.K;
    float *x = smem, *z = x + K * T, *r = z + K * T, *b = r + M * T;
    const unsigned n = blockIdx.x / p.tiles, tile = blockIdx.x - n * p.tiles;
    const int G = T / FR;                       // lanes per row
    const int t0 = FR * (threadIdx.x % G), row0 = threadIdx.x / G, rows = THREADS / G;
    const unsigned f0 = tile * T + t0;          // the lane's first frame
    unsigned Fn = p.F;
    if (p.frames) {
        const long long v = p.frames[n];
        Fn = v < 0 ? 0u : (v > (long long)p.F ? p.F : (unsigned)v);
    }
    const unsigned *hdr = p.plan;
    const float *d = reinterpret_cast<const float *>(hdr + hdr[H_D]);
    const float *cinv = reinterpret_cast<const float *>(hdr + hdr[H_CINV]);
    const float *beta = reinterpret_cast<const float *>(hdr + hdr[H_BETA]);
    const unsigned *tab = hdr + hdr[H_RBAND];
    if (TAB) {
        unsigned *lt = reinterpret_cast<unsigned *>(b + M * T);
        const int words = 2 * M + 2 * K + (int)hdr[H_NNZR] + (int)hdr[H_NNZC];
        for (int i = threadIdx.x; i < words; i += THREADS) lt[i] = tab[i];
        tab = lt;                               // visible behind the first barrier below
    }
    const unsigned *rband = tab, *cband = tab + 2 * M;
    const float *rvals = reinterpret_cast<const float *>(cband + 2 * K);
    const float *cvals = rvals + hdr[H_NNZR];
    const float step = __uint_as_float(hdr[H_STEP]);
    float *out = p.out + (size_t)n * K * p.F + f0;

    // b = d max(lin, 0); a frame behind the item's length is never read and iterates on zeros
    const float *Y = p.Y + (size_t)n * M * p.F + f0;
    for (int m = row0; m < M; m += rows) {
        Frames<FR> v;
        const float dm = d[m];
#pragma unroll
        for (int e = 0; e < FR; ++e)
            v.v[e] = f0 + e < Fn ? dm * fmaxf(undo_log(Y[(size_t)m * p.F + e], p.log_kind, p.log_offset), 0.f) : 0.f;
        lds_put<FR>(b + m * T + t0, v);
    }
    __syncthreads();
    // the flat-band guess x0 = cinv A^T b
    for (int k = row0; k < K; k += rows) {
        Frames<FR> v = band_dot<FR>(band_of(cband, k, K), cvals, b, T, t0);
        const float ck = cinv[k];
#pragma unroll
        for (int e = 0; e < FR; ++e) v.v[e] = ck * v.v[e];
        lds_put<FR>(x + k * T + t0, v);
        lds_put<FR>(z + k * T + t0, v);
    }
    __syncthreads();
    // A v - b into r; the band of a lane's next row is asked for before the sum over this one starts
    auto residual = [&](const float *v) {
        u32x2 h = band_of(rband, row0, M);
        for (int m = row0; m < M; m += rows) {
            const u32x2 hn = band_of(rband, m + rows, M);
            Frames<FR> acc = band_dot<FR>(h, rvals, v, T, t0);
            const Frames<FR> bm = lds_get<FR>(b + m * T + t0);
#pragma unroll
            for (int e = 0; e < FR; ++e) acc.v[e] -= bm.v[e];
            lds_put<FR>(r + m * T + t0, acc);
            h = hn;
        }
    };
    for (int i = 0; i < p.n_iter; ++i) {
        const float be = beta[i];
        residual(z);
        __syncthreads();
        u32x2 h = band_of(cband, row0, K);
        for (int k = row0; k < K; k += rows) {
            const u32x2 hn = band_of(cband, k + rows, K);
            const Frames<FR> g = band_dot<FR>(h, cvals, r, T, t0);
            const Frames<FR> xo = lds_get<FR>(x + k * T + t0), zo = lds_get<FR>(z + k * T + t0);
            Frames<FR> xn, zn;
#pragma unroll
            for (int e = 0; e < FR; ++e) {
                xn.v[e] = fmaxf(__builtin_fmaf(-step, g.v[e], zo.v[e]), 0.f);
                zn.v[e] = __builtin_fmaf(be, xn.v[e] - xo.v[e], xn.v[e]);
            }
            lds_put<FR>(x + k * T + t0, xn);
            lds_put<FR>(z + k * T + t0, zn);
            h = hn;
        }
        __syncthreads();
    }
    for (int k = row0; k < K; k += rows) {
        const Frames<FR> xk = lds_get<FR>(x + k * T + t0);
#pragma unroll
        for (int e = 0; e < FR; ++e)
            if (f0 + e < p.F) out[(size_t)k * p.F + e] = f0 + e < Fn ? xk.v[e] : 0.f;
    }
    if (p.resid) {                              // |A x - b| / |b| of the frame, the sums in ascending m
        residual(x);
        __syncthreads();
        if (row0 == 0) {
            for (int e = 0; e < FR; ++e) {
                if (f0 + e >= p.F) break;
                float rr = 0.f, bb = 0.f;
                for (int m = 0; m < M; ++m) {
                    rr = __builtin_fmaf(r[m * T + t0 + e], r[m * T + t0 + e], rr);
                    bb = __builtin_fmaf(b[m * T + t0 + e], b[m * T + t0 + e], bb);
                }
                p.resid[(size_t)n * p.F + f0 + e] = f0 + e < Fn && bb > 0.f ? sqrtf(rr / bb) : 0.f;
            }
        }
    }
}

__global__ __launch_bounds__(THREADS) void mel_inverse_kernel(MiParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const unsigned *hdr = p.plan;
    if (hdr[H_MAGIC] != MAGIC || (int)hdr[H_M] != p.M || (int)hdr[H_K] != p.K || p.n_iter > (int)hdr[H_NMAX]) {
        // not a plan, one of another filterbank size, or one with fewer momentum factors than iterations asked for: loud, not wrong.
        // Nothing of the plan beyond these four words is read.
        const unsigned n = blockIdx.x / p.tiles, tile = blockIdx.x - n * p.tiles;
        const unsigned f = tile * p.T + threadIdx.x % p.T;
        if (f < p.F) {
            for (int k = threadIdx.x / p.T; k < p.K; k += THREADS / p.T) p.out[((size_t)n * p.K + k) * p.F + f] = __builtin_nanf("");
            if (p.resid && threadIdx.x < p.T) p.resid[(size_t)n * p.F + f] = __builtin_nanf("");
        }
        return;
    }
    const int words = 2 * p.M + 2 * p.K + (int)hdr[H_NNZR] + (int)hdr[H_NNZC];
    const bool tab = words <= p.tab_cap;
    if (p.T >= 4) {
        if (tab) mel_inverse_body<true, 4>(p, smem);
        else mel_inverse_body<false, 4>(p, smem);
    } else {
        if (tab) mel_inverse_body<true, 2>(p, smem);
        else mel_inverse_body<false, 2>(p, smem);
    }
}

}  // namespace

extern "C" int psnd_mel_inverse_tile(int M, int K) { return tile_of(M, K); }

extern "C" int psnd_mel_inverse_max_iter(void) { return MAX_ITER; }

extern "C" size_t psnd_mel_inverse_plan_bytes(int M, int K) {
    if (M <= 0 || K <= 0 || M > MAX_M || K > MAX_K) return 0;
    return (size_t)layout(M, K).words * 4;
}

extern "C" int psnd_mel_inverse_plan_build(int M, int K, const float *W, int n_iter_max, void *plan_host) {
#pragma clang fp contract(off)
    if (!W || !plan_host || M <= 0 || K <= 0 || n_iter_max < 0) PSND_FAIL(PSND_E_ARG, "mel_inverse_plan_build: bad arguments");
    if (M > MAX_M || K > MAX_K)
        PSND_FAIL(PSND_E_UNSUPPORTED, "mel_inverse_plan_build: M=%d K=%d: the kernel serves M <= %d filters and K <= %d bins", M, K, MAX_M, MAX_K);
    if (n_iter_max > MAX_ITER)
        PSND_FAIL(PSND_E_UNSUPPORTED, "mel_inverse_plan_build: n_iter_max=%d: the plan holds at most %d momentum factors", n_iter_max, MAX_ITER);
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k) {
            const float w = W[(size_t)m * K + k];
            if (!(w >= 0.f) || !isfinite(w))
                PSND_FAIL(PSND_E_ARG, "mel_inverse_plan_build: weight [%d, %d] = %g: the filterbank must be finite and >= 0", m, k, (double)w);
        }
    const Layout l = layout(M, K);
    unsigned *hdr = static_cast<unsigned *>(plan_host);
    memset(hdr, 0, (size_t)l.words * 4);
    double *f64 = reinterpret_cast<double *>(hdr + l.f64);       // step, L, d[M], cinv[K]
    float *d32 = reinterpret_cast<float *>(hdr + l.d), *c32 = reinterpret_cast<float *>(hdr + l.cinv);
    float *beta = reinterpret_cast<float *>(hdr + l.beta), *A = reinterpret_cast<float *>(hdr + l.A);
    double *d = f64 + 2, *cinv = d + M;
    for (int m = 0; m < M; ++m) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) s += (double)W[(size_t)m * K + k];
        d[m] = s > 0.0 ? 1.0 / s : 0.0;
        d32[m] = (float)d[m];
        for (int k = 0; k < K; ++k) A[(size_t)m * K + k] = (float)(d[m] * (double)W[(size_t)m * K + k]);
    }
    std::vector<double> c(K);
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int m = 0; m < M; ++m) s += (double)A[(size_t)m * K + k];
        c[k] = s;
        cinv[k] = s > 0.0 ? 1.0 / s : 0.0;
        c32[k] = (float)cinv[k];
    }
    double L = 0.0;
    for (int m = 0; m < M; ++m) {
        double s = 0.0;
        for (int k = 0; k < K; ++k) {
            const double prod = (double)A[(size_t)m * K + k] * c[k];
            s += prod;
        }
        if (s > L) L = s;
    }
    const double step = L > 0.0 ? 1.0 / L : 0.0;
    f64[0] = step, f64[1] = L;
    double tp = 1.0;
    for (int i = 0; i < n_iter_max; ++i) {
        const double tn = (1.0 + sqrt(1.0 + 4.0 * tp * tp)) / 2.0;
        beta[i] = (float)((tp - 1.0) / tn);
        tp = tn;
    }
    // the bands: first to last non-zero weight of a row / a column, packed one after the other
    unsigned *rband = hdr + l.rband, *cband = hdr + l.cband;
    float *vals = reinterpret_cast<float *>(hdr + l.vals);
    unsigned at = 0;
    for (int m = 0; m < M; ++m) {
        int lo = K, hi = 0;
        for (int k = 0; k < K; ++k)
            if (A[(size_t)m * K + k] != 0.f) lo = k < lo ? k : lo, hi = k + 1;
        if (hi <= lo) lo = hi = 0;
        rband[2 * m] = (unsigned)lo | ((unsigned)(hi - lo) << 16), rband[2 * m + 1] = at;
        for (int k = lo; k < hi; ++k) vals[at++] = A[(size_t)m * K + k];
    }
    const unsigned nnzr = at;
    for (int k = 0; k < K; ++k) {
        int lo = M, hi = 0;
        for (int m = 0; m < M; ++m)
            if (A[(size_t)m * K + k] != 0.f) lo = m < lo ? m : lo, hi = m + 1;
        if (hi <= lo) lo = hi = 0;
        cband[2 * k] = (unsigned)lo | ((unsigned)(hi - lo) << 16), cband[2 * k + 1] = at - nnzr;
        for (int m = lo; m < hi; ++m) vals[at++] = A[(size_t)m * K + k];
    }
    const float stepf = (float)step;
    hdr[H_MAGIC] = MAGIC, hdr[H_M] = M, hdr[H_K] = K, hdr[H_NMAX] = n_iter_max, hdr[H_NNZR] = nnzr, hdr[H_NNZC] = at - nnzr;
    memcpy(&hdr[H_STEP], &stepf, 4);
    hdr[H_D] = l.d, hdr[H_CINV] = l.cinv, hdr[H_BETA] = l.beta, hdr[H_RBAND] = l.rband, hdr[H_CBAND] = l.cband;
    hdr[H_RVALS] = l.vals, hdr[H_CVALS] = l.vals + nnzr, hdr[H_A] = l.A, hdr[H_F64] = l.f64, hdr[H_WORDS] = l.words;
    return PSND_OK;
}

extern "C" int psnd_mel_inverse(const float *mel, int64_t N, int64_t F, int M, int K, const void *plan, int log_kind, float log_offset,
                                int n_iter, const int64_t *frames, float *out, float *resid, void *stream) {
    if (N < 0 || F < 0 || M <= 0 || K <= 0 || n_iter < 0)
        PSND_FAIL(PSND_E_ARG, "mel_inverse: N=%lld F=%lld M=%d K=%d n_iter=%d", (long long)N, (long long)F, M, K, n_iter);
    if (log_kind != PSND_LOG_NONE && log_kind != PSND_LOG_E && log_kind != PSND_LOG_10) PSND_FAIL(PSND_E_ARG, "mel_inverse: log_kind=%d", log_kind);
    if (M > MAX_M || K > MAX_K)
        PSND_FAIL(PSND_E_UNSUPPORTED, "mel_inverse: M=%d K=%d: the kernel serves M <= %d filters and K <= %d bins", M, K, MAX_M, MAX_K);
    if (n_iter > MAX_ITER) PSND_FAIL(PSND_E_UNSUPPORTED, "mel_inverse: n_iter=%d: a plan holds at most %d momentum factors", n_iter, MAX_ITER);
    if (N == 0 || F == 0) return PSND_OK;
    if (!mel || !plan || !out) PSND_FAIL(PSND_E_ARG, "mel_inverse: null pointer");
    if (F >= 0x7fffffffll / K) PSND_FAIL(PSND_E_SHAPE, "mel_inverse: K=%d F=%lld is 2^31 or more elements per item", K, (long long)F);
    const int T = tile_of(M, K);
    const int64_t tiles = (F + T - 1) / T;
    if (tiles > 0x7fffffffll / N) PSND_FAIL(PSND_E_SHAPE, "mel_inverse: N=%lld F=%lld is more than 2^31 - 1 workgroups", (long long)N, (long long)F);
    MiParams p;
    p.Y = mel, p.plan = static_cast<const unsigned *>(plan), p.frames = reinterpret_cast<const long long *>(frames);
    p.out = out, p.resid = resid, p.F = (unsigned)F, p.tiles = (unsigned)tiles;
    p.M = M, p.K = K, p.T = T, p.n_iter = n_iter, p.log_kind = log_kind, p.log_offset = log_offset;
    const int state = T * (2 * K + 2 * M);
    p.tab_cap = LDS_WORDS - state < TAB_WORDS ? LDS_WORDS - state : TAB_WORDS;
    if (2 * M + 2 * K > p.tab_cap) p.tab_cap = 0;        // the band tables alone do not fit (128 x 2049): no LDS is asked for them
    const size_t lds = (size_t)(state + p.tab_cap) * sizeof(float);
    hipLaunchKernelGGL(mel_inverse_kernel, dim3((unsigned)(N * tiles)), dim3(THREADS), lds, static_cast<hipStream_t>(stream), p);
    PSND_CHECK_LAUNCH("mel_inverse");
    return PSND_OK;
}
