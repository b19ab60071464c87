// psnd_separation.hip - SNR / SI-SDR / SD-SDR with permutation-invariant matching, their gradient, and mixing at a wanted SNR on (B, S, T)
// fp32 rows on gfx950.  The definition is in include/psnd.h.  The reference names the tasks (VoiceBank, DSD100 / MUSDB18 / MedleyDB) and
// has no waveform-domain objective or score.
//
// Every metric of the family is a function of the second moments of the estimate and target rows, so one read of the 2 S rows of an item
// gives the whole S x S pair matrix:
//   1  sep_moment_kernel<S>  a workgroup of 256 lanes owns one span of 8192 samples of ALL 2 S rows of an item.  The span is cut into a scalar
//                            head (up to the first 16-byte boundary of the item's first estimate row), quads read by 16-byte loads (quad q by
//                            lane q mod 256) and a scalar tail.  A lane keeps S^2 + 4 S fp64 accumulators in registers: sum e_i, sum s_j,
//                            sum e_i^2, sum s_j^2, sum e_i s_j.  Lanes fold by shuffles, the four waves through LDS in ascending order, and
//                            part[item][span][moment] is stored once (the last slot of a span: 1.0 where a sample was not finite; it
//                            entered the sums as 0).  Spans that start behind the item's length store nothing and are never read.
//   2  sep_item_kernel       one wave per item: lane m adds the partials of moment m in ascending span order; the S^2 pair values in fp64,
//                            rounded once to fp32; lane 0 walks the S! permutations in lexicographic order; value, perm, pair, stats.
//   3  sep_loss_kernel       one workgroup: -(1 / (B S)) sum value by per-lane sums and a fixed tree, and the NaN flag.
// sep_bwd_kernel is elementwise: every thread forms the six coefficients of its row from stats and perm (a few dozen fp64 operations) and
// writes g_est[b][i] and g_target[b][p(i)] - p is a permutation, so every element of both is written once.
// psnd_snr_gain is launch 1 with S = 1 plus snr_gain_kernel (a lane per row); psnd_mix_rows is the sibling of psnd_gain_rows.
// No atomics, no workgroup waits on another inside a launch, nothing read back by the host.
#include "psnd_common.h"
#include <math.h>

namespace {

constexpr int LANES = 256;
constexpr int WAVES = LANES / 64;
constexpr int SPAN = 8192;                              // samples of a row per workgroup of the moment launch
constexpr int MAX_S = 4;
constexpr int MAX_NM = MAX_S * MAX_S + 4 * MAX_S;
constexpr int ROW_PER = 4096;                           // samples per workgroup of the elementwise kernels
constexpr int ROW_QUADS = ROW_PER / (4 * LANES);

__host__ __device__ constexpr int n_mom(int S) { return S * S + 4 * S; }

__device__ __forceinline__ bool non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ long long item_len(const long long *lengths, long long item, long long T) {
    if (!lengths) return T;
    const long long v = lengths[item];
    return v < 0 ? 0 : (v > T ? T : v);
}

template <int S>
struct Acc {
    double se[S], ss[S], see[S], sss[S], ses[S * S];
};

// one sample of every row
template <int S>
__device__ __forceinline__ void take(Acc<S> &a, const float (&e)[S], const float (&s)[S], bool &bad) {
    double de[S], ds[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const bool ne = non_finite(e[i]), ns = non_finite(s[i]);
        bad |= ne | ns;
        de[i] = ne ? 0.0 : (double)e[i];
        ds[i] = ns ? 0.0 : (double)s[i];
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
        a.se[i] += de[i];
        a.ss[i] += ds[i];
        a.see[i] = fma(de[i], de[i], a.see[i]);
        a.sss[i] = fma(ds[i], ds[i], a.sss[i]);
    }
#pragma unroll
    for (int i = 0; i < S; ++i)
#pragma unroll
        for (int j = 0; j < S; ++j) a.ses[i * S + j] = fma(de[i], ds[j], a.ses[i * S + j]);
}

__device__ __forceinline__ double wave_sum(double v) {   // lane 0 holds the sum
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// ---- launch 1 -----------------------------------------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(LANES) void sep_moment_kernel(const float *est, const float *tgt, long long T, const long long *lengths, int spans,
                                                           double *part) {
    constexpr int NM = n_mom(S);
    __shared__ double red[WAVES][NM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long item = blockIdx.x / spans;
    const int span = (int)(blockIdx.x % spans);
    const long long b0 = (long long)span * SPAN;
    const long long L = item_len(lengths, item, T);
    if (b0 >= L) return;                                // the whole workgroup: nothing behind the length is read, and launch 2 skips the slot
    const int n = (int)((L - b0 < SPAN) ? L - b0 : SPAN);          // samples of this span, 1 .. SPAN: all of them lie before L <= T
    const float *e0 = est + (size_t)item * S * T + b0;
    const float *s0 = tgt + (size_t)item * S * T + b0;
    int head = (int)((16u - (unsigned)((uintptr_t)e0 & 15u)) & 15u) >> 2;
    if (head > n) head = n;
    const int quads = (n - head) >> 2;
    const int tail0 = head + 4 * quads;                 // [tail0, n): at most three samples
    Acc<S> a = {};
    bool bad = false;
    if (tid < head + (n - tail0)) {                     // at most six lanes
        const int k = tid < head ? tid : tail0 + (tid - head);
        float e1[S], s1[S];
#pragma unroll
        for (int i = 0; i < S; ++i) e1[i] = e0[(size_t)i * T + k], s1[i] = s0[(size_t)i * T + k];
        take<S>(a, e1, s1, bad);
    }
#pragma unroll 2
    for (int q = tid; q < quads; q += LANES) {
        const int k = head + 4 * q;                     // k + 3 < n
        f32x4 ev[S], sv[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            ev[i] = *reinterpret_cast<const f32x4_u *>(e0 + (size_t)i * T + k);
            sv[i] = *reinterpret_cast<const f32x4_u *>(s0 + (size_t)i * T + k);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float e1[S], s1[S];
#pragma unroll
            for (int i = 0; i < S; ++i) e1[i] = ev[i][c], s1[i] = sv[i][c];
            take<S>(a, e1, s1, bad);
        }
    }
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const double v0 = wave_sum(a.se[i]), v1 = wave_sum(a.ss[i]), v2 = wave_sum(a.see[i]), v3 = wave_sum(a.sss[i]);
        if (lane == 0) red[wave][i] = v0, red[wave][S + i] = v1, red[wave][2 * S + i] = v2, red[wave][3 * S + i] = v3;
    }
#pragma unroll
    for (int i = 0; i < S * S; ++i) {
        const double v = wave_sum(a.ses[i]);
        if (lane == 0) red[wave][4 * S + i] = v;
    }
    const int any_bad = __syncthreads_or(bad);
    double *o = part + ((size_t)item * spans + span) * (NM + 1);
    if (tid < NM) o[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    if (tid == NM) o[NM] = any_bad ? 1.0 : 0.0;
}

// ---- the pair value and its derivatives -----------------------------------------------------------------------------------------------------
struct Cent {
    double ee, ss, es, eb, sb;                          // the (centred) moments of a pair and the means that were taken out (0 without)
};

// m: the moments of an item in the order of `stats`
__device__ __forceinline__ Cent centred(const double *m, int S, int i, int j, double L, int zero_mean) {
    Cent c = {m[2 * S + i], m[3 * S + j], m[4 * S + i * S + j], 0.0, 0.0};
    if (zero_mean && L > 0.0) {
        c.eb = m[i] / L, c.sb = m[S + j] / L;
        c.ee = fmax(c.ee - m[i] * m[i] / L, 0.0);
        c.ss = fmax(c.ss - m[S + j] * m[S + j] / L, 0.0);
        c.es = c.es - m[i] * m[S + j] / L;
    }
    return c;
}

__device__ __forceinline__ double pair_value(int kind, const Cent &c, double eps) {
    if (kind == 0) {
        const double N = fmax(c.ss - 2.0 * c.es + c.ee, 0.0);
        return 10.0 * log10((c.ss + eps) / (N + eps));
    }
    const double al = (c.es + eps) / (c.ss + eps);
    const double Tg = al * al * c.ss;
    const double N = fmax(kind == 1 ? Tg - 2.0 * al * c.es + c.ee : c.ss - 2.0 * c.es + c.ee, 0.0);
    return 10.0 * log10((Tg + eps) / (N + eps));
}

struct Coef {
    double Ae, Be, Ce, As, Bs, Cs;                      // d v / d e[t] = Ae e + Be s + Ce, d v / d s[t] = As e + Bs s + Cs
};

__device__ __forceinline__ Coef pair_grad(int kind, const Cent &c, double eps) {
    const double k10 = 4.342944819032518;               // 10 / ln 10
    double gee, ges, gss;                               // d v / d ee, es, ss
    if (kind == 0) {
        const double N = c.ss - 2.0 * c.es + c.ee;
        const double gN = N >= 0.0 ? -k10 / (N + eps) : 0.0;
        gee = gN, ges = -2.0 * gN, gss = k10 / (c.ss + eps) + gN;
    } else {
        const double q = 1.0 / (c.ss + eps);
        const double al = (c.es + eps) * q;
        const double Tg = al * al * c.ss;
        const double gT = k10 / (Tg + eps);
        if (kind == 1) {
            const double N = Tg - 2.0 * al * c.es + c.ee;
            const double gN = N >= 0.0 ? -k10 / (N + eps) : 0.0;
            const double ga = gT * 2.0 * al * c.ss + gN * (2.0 * al * c.ss - 2.0 * c.es);
            gee = gN, ges = -2.0 * al * gN + ga * q, gss = (gT + gN) * al * al - ga * al * q;
        } else {
            const double N = c.ss - 2.0 * c.es + c.ee;
            const double gN = N >= 0.0 ? -k10 / (N + eps) : 0.0;
            const double ga = gT * 2.0 * al * c.ss;
            gee = gN, ges = -2.0 * gN + ga * q, gss = gT * al * al + gN - ga * al * q;
        }
    }
    return Coef{2.0 * gee, ges, -(2.0 * gee * c.eb + ges * c.sb), ges, 2.0 * gss, -(ges * c.eb + 2.0 * gss * c.sb)};
}

// ---- launch 2 -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool next_perm(int *p, int S) {        // the next permutation in lexicographic order; false behind the last
    int i = S - 2;
    while (i >= 0 && p[i] > p[i + 1]) --i;
    if (i < 0) return false;
    int j = S - 1;
    while (p[j] < p[i]) --j;
    int t = p[i];
    p[i] = p[j], p[j] = t;
    for (int lo = i + 1, hi = S - 1; lo < hi; ++lo, --hi) t = p[lo], p[lo] = p[hi], p[hi] = t;
    return true;
}

__global__ __launch_bounds__(64) void sep_item_kernel(int S, long long T, const long long *lengths, int spans, int kind, int zero_mean, double eps,
                                                      int pit, const double *part, double *stats, float *value, int *perm, float *pair) {
    __shared__ double mom[MAX_NM + 1];
    __shared__ float pv[MAX_S * MAX_S];
    __shared__ int p[MAX_S], best[MAX_S];
    const int tid = threadIdx.x;
    const int NM = n_mom(S);
    const long long item = blockIdx.x;
    const long long L = item_len(lengths, item, T);
    const int used = (int)((L + SPAN - 1) / SPAN);      // the spans launch 1 has written: those that start before L
    if (tid <= NM) {
        const double *q = part + (size_t)item * spans * (NM + 1) + tid;
        double v = 0.0;
        for (int sp = 0; sp < used; ++sp) v += q[(size_t)sp * (NM + 1)];
        mom[tid] = v;
    }
    __syncthreads();
    const bool bad = mom[NM] != 0.0;
    double *st = stats + (size_t)item * (NM + 2);
    if (tid < NM) st[tid] = mom[tid];
    if (tid == NM) st[NM] = (double)L;
    if (tid == NM + 1) st[NM + 1] = bad ? 1.0 : 0.0;
    if (tid < S * S) {
        const int i = tid / S, j = tid % S;
        float v = __uint_as_float(0x7fc00000u);
        if (!bad && (pit || pair || i == j)) v = (float)pair_value(kind, centred(mom, S, i, j, (double)L, zero_mean), eps);
        pv[tid] = v;
        if (pair) pair[(size_t)item * S * S + tid] = v;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 0; i < S; ++i) p[i] = best[i] = i;
        if (pit && !bad) {
            double top = 0.0;
            bool first = true;
            do {
                double s = 0.0;
                for (int i = 0; i < S; ++i) s += (double)pv[i * S + p[i]];
                if (first || s > top) {
                    top = s, first = false;
                    for (int i = 0; i < S; ++i) best[i] = p[i];
                }
            } while (next_perm(p, S));
        }
        for (int i = 0; i < S; ++i) {
            value[(size_t)item * S + i] = pv[i * S + best[i]];
            perm[(size_t)item * S + i] = best[i];
        }
    }
}

// ---- launch 3 -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void sep_loss_kernel(const float *value, long long n, float *loss, float *nan_flag) {
    __shared__ double sv[LANES];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < n; i += LANES) s += (double)value[i];
    sv[tid] = s;
    __syncthreads();
    for (int d = LANES / 2; d > 0; d >>= 1) {
        if (tid < d) sv[tid] += sv[tid + d];
        __syncthreads();
    }
    if (tid == 0) {
        const float l = (float)(-sv[0] / (double)n);
        if (loss) loss[0] = l;
        if (nan_flag) nan_flag[0] = l != l ? 1.f : 0.f;
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void sep_bwd_kernel(const float *est, const float *tgt, int S, long long T, int chunks, int kind, int zero_mean,
                                                        double eps, const double *stats, const int *perm, const float *g_loss,
                                                        const float *g_value, double inv_n, float *g_est, float *g_tgt) {
    const long long row = blockIdx.x / chunks;          // item S + i
    const long long c0 = (long long)(blockIdx.x % chunks) * ROW_PER;
    const long long item = row / S;
    const int i = (int)(row % S);
    const int NM = n_mom(S);
    const double *st = stats + (size_t)item * (NM + 2);
    long long L = (long long)st[NM];
    L = L < 0 ? 0 : (L > T ? T : L);
    int j = perm[row];
    j = j < 0 ? 0 : (j >= S ? S - 1 : j);               // whatever the buffers hold, nothing outside the item is touched
    const double G = (g_value ? (double)g_value[row] : 0.0) - (g_loss ? (double)g_loss[0] * inv_n : 0.0);
    Coef k = pair_grad(kind, centred(st, S, i, j, (double)L, zero_mean), eps);
    if (st[NM + 1] != 0.0) k.Ae = k.Be = k.Ce = k.As = k.Bs = k.Cs = __longlong_as_double(0x7ff8000000000000ll);
    k.Ae *= G, k.Be *= G, k.Ce *= G, k.As *= G, k.Bs *= G, k.Cs *= G;
    const float *er = est + (size_t)row * T;
    const float *sr = tgt + ((size_t)item * S + j) * T;
    float *ge = g_est + (size_t)row * T;
    float *gs = g_tgt ? g_tgt + ((size_t)item * S + j) * T : nullptr;
#pragma unroll
    for (int q = 0; q < ROW_QUADS; ++q) {
        const long long t = c0 + 4ll * (threadIdx.x + q * LANES);
        if (t >= T) break;
        if (t + 3 < L) {                                // t + 3 < L <= T
            const f32x4 e = *reinterpret_cast<const f32x4_u *>(er + t);
            const f32x4 s = *reinterpret_cast<const f32x4_u *>(sr + t);
            f32x4 oe, os;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                oe[c] = (float)fma(k.Ae, (double)e[c], fma(k.Be, (double)s[c], k.Ce));
                os[c] = (float)fma(k.As, (double)e[c], fma(k.Bs, (double)s[c], k.Cs));
            }
            *reinterpret_cast<f32x4_u *>(ge + t) = oe;
            if (gs) *reinterpret_cast<f32x4_u *>(gs + t) = os;
        } else {
            for (int c = 0; c < 4 && t + c < T; ++c) {
                float oe = 0.f, os = 0.f;
                if (t + c < L) {
                    const double e = (double)er[t + c], s = (double)sr[t + c];
                    oe = (float)fma(k.Ae, e, fma(k.Be, s, k.Ce));
                    os = (float)fma(k.As, e, fma(k.Bs, s, k.Cs));
                }
                ge[t + c] = oe;
                if (gs) gs[t + c] = os;
            }
        }
    }
}

// ---- mixing at an SNR -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void snr_gain_kernel(long long R, long long T, const long long *lengths, int spans, const double *part,
                                                         const float *snr, int per_row, float *gain) {
    constexpr int NP = n_mom(1) + 1;                    // Se, Ss, See, Sss, Ses, flag
    const long long r = (long long)blockIdx.x * LANES + threadIdx.x;
    if (r >= R) return;
    const long long L = item_len(lengths, r, T);
    const int used = (int)((L + SPAN - 1) / SPAN);
    const double *q = part + (size_t)r * spans * NP;
    double xx = 0.0, zz = 0.0, bad = 0.0;
    for (int sp = 0; sp < used; ++sp) xx += q[(size_t)sp * NP + 2], zz += q[(size_t)sp * NP + 3], bad += q[(size_t)sp * NP + 5];
    float g = 0.f;
    if (bad == 0.0 && xx > 0.0 && zz > 0.0) g = (float)(sqrt(xx / zz) * pow(10.0, -(double)snr[per_row ? r : 0] / 20.0));
    gain[r] = g;
}

__global__ __launch_bounds__(LANES) void mix_rows_kernel(const float *x, const float *z, long long T, const long long *lengths, int chunks,
                                                         const float *gain, float *y) {
    const long long row = blockIdx.x / chunks;
    const long long c0 = (long long)(blockIdx.x % chunks) * ROW_PER;
    const float g = gain[row];
    const long long L = g != 0.f ? item_len(lengths, row, T) : 0;      // g = 0 copies the row: 0 times a non-finite noise sample is not 0
    const float *xr = x + (size_t)row * T;
    const float *zr = z + (size_t)row * T;
    float *yr = y + (size_t)row * T;
#pragma unroll
    for (int q = 0; q < ROW_QUADS; ++q) {
        const long long t = c0 + 4ll * (threadIdx.x + q * LANES);
        if (t >= T) break;
        if (t + 3 < T) {
            f32x4 v = *reinterpret_cast<const f32x4_u *>(xr + t);
            if (t < L) {                                // nothing of the noise is read behind the length
                if (t + 3 < L) {
                    const f32x4 w = *reinterpret_cast<const f32x4_u *>(zr + t);
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[c] = fmaf(g, w[c], v[c]);
                } else {
                    for (int c = 0; c < 4 && t + c < L; ++c) v[c] = fmaf(g, zr[t + c], v[c]);
                }
            }
            *reinterpret_cast<f32x4_u *>(yr + t) = v;
        } else {
            for (int c = 0; c < 4 && t + c < T; ++c) yr[t + c] = t + c < L ? fmaf(g, zr[t + c], xr[t + c]) : xr[t + c];
        }
    }
}

inline long long n_spans(long long T) { return T > 0 ? (T + SPAN - 1) / SPAN : 0; }
inline long long n_chunks(long long T) { return (T + ROW_PER - 1) / ROW_PER; }

int launch_moments(const float *est, const float *tgt, long long B, int S, long long T, const long long *len, double *part, hipStream_t st) {
    const int spans = (int)n_spans(T);
    const dim3 grid((unsigned)(B * spans)), block(LANES);
    switch (S) {
        case 1: hipLaunchKernelGGL(sep_moment_kernel<1>, grid, block, 0, st, est, tgt, T, len, spans, part); break;
        case 2: hipLaunchKernelGGL(sep_moment_kernel<2>, grid, block, 0, st, est, tgt, T, len, spans, part); break;
        case 3: hipLaunchKernelGGL(sep_moment_kernel<3>, grid, block, 0, st, est, tgt, T, len, spans, part); break;
        default: hipLaunchKernelGGL(sep_moment_kernel<4>, grid, block, 0, st, est, tgt, T, len, spans, part); break;
    }
    PSND_CHECK_LAUNCH("sep_metric (moments)");
    return PSND_OK;
}

// the checks the two directions share; 1: nothing to do
int check_geometry(const char *who, int64_t B, int64_t S, int64_t T, int kind, int zero_mean, double eps) {
    if (kind < 0 || kind > 2) PSND_FAIL(PSND_E_ARG, "%s: kind=%d (0 snr, 1 si_sdr, 2 sd_sdr)", who, kind);
    if (zero_mean != 0 && zero_mean != 1) PSND_FAIL(PSND_E_ARG, "%s: zero_mean=%d", who, zero_mean);
    if (!(eps >= 0.0) || !isfinite(eps)) PSND_FAIL(PSND_E_ARG, "%s: eps=%g (finite, >= 0)", who, eps);
    if (S < 1) PSND_FAIL(PSND_E_ARG, "%s: S=%lld", who, (long long)S);
    if (B < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "%s: B=%lld T=%lld", who, (long long)B, (long long)T);
    if (S > MAX_S) PSND_FAIL(PSND_E_UNSUPPORTED, "%s: S=%lld, at most %d sources per item", who, (long long)S, MAX_S);
    return PSND_OK;
}

}  // namespace

extern "C" int64_t psnd_sep_span(void) { return SPAN; }
extern "C" int64_t psnd_sep_max_sources(void) { return MAX_S; }

extern "C" size_t psnd_sep_scratch_bytes(int64_t B, int64_t S, int64_t T) {
    if (B <= 0 || S < 1 || S > MAX_S || T <= 0) return 0;
    return (size_t)B * (size_t)n_spans(T) * (size_t)(n_mom((int)S) + 1) * sizeof(double);
}

extern "C" int64_t psnd_sep_stats_doubles(int64_t B, int64_t S) {
    if (B <= 0 || S < 1 || S > MAX_S) return 0;
    return B * (int64_t)(n_mom((int)S) + 2);
}

extern "C" int psnd_sep_metric_fwd(const float *est, const float *target, int64_t B, int64_t S, int64_t T, const int64_t *lengths, int kind,
                                   int zero_mean, double eps, int pit, void *scratch, double *stats, float *value, int *perm, float *pair,
                                   float *loss, float *nan_flag, void *stream) {
    const int rc = check_geometry("sep_metric_fwd", B, S, T, kind, zero_mean, eps);
    if (rc != PSND_OK) return rc;
    if (pit != 0 && pit != 1) PSND_FAIL(PSND_E_ARG, "sep_metric_fwd: pit=%d", pit);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (B == 0 || T == 0) {                             // the empty sum
        if (loss && hipMemsetAsync(loss, 0, sizeof(float), st) != hipSuccess) PSND_FAIL(PSND_E_HIP, "sep_metric_fwd: memset of the loss");
        if (nan_flag && hipMemsetAsync(nan_flag, 0, sizeof(float), st) != hipSuccess) PSND_FAIL(PSND_E_HIP, "sep_metric_fwd: memset of the flag");
        return PSND_OK;
    }
    if (!est || !target || !scratch || !stats || !value || !perm) PSND_FAIL(PSND_E_ARG, "sep_metric_fwd: null pointer");
    if ((uintptr_t)scratch % 8 || (uintptr_t)stats % 8) PSND_FAIL(PSND_E_ARG, "sep_metric_fwd: scratch and stats must be 8-byte aligned");
    const long long spans = n_spans(T);
    if (B > 0x7fffffff / spans || B * S > 0x7fffffff)
        PSND_FAIL(PSND_E_SHAPE, "sep_metric_fwd: B=%lld T=%lld is more than 2^31 - 1 workgroups", (long long)B, (long long)T);
    const long long *len = reinterpret_cast<const long long *>(lengths);
    double *part = static_cast<double *>(scratch);
    const int rm = launch_moments(est, target, B, (int)S, T, len, part, st);
    if (rm != PSND_OK) return rm;
    hipLaunchKernelGGL(sep_item_kernel, dim3((unsigned)B), dim3(64), 0, st, (int)S, (long long)T, len, (int)spans, kind, zero_mean, eps, pit,
                       (const double *)part, stats, value, perm, pair);
    PSND_CHECK_LAUNCH("sep_metric (items)");
    if (loss || nan_flag) {
        hipLaunchKernelGGL(sep_loss_kernel, dim3(1), dim3(LANES), 0, st, (const float *)value, (long long)(B * S), loss, nan_flag);
        PSND_CHECK_LAUNCH("sep_metric (loss)");
    }
    return PSND_OK;
}

extern "C" int psnd_sep_metric_bwd(const float *est, const float *target, int64_t B, int64_t S, int64_t T, int kind, int zero_mean, double eps,
                                   const double *stats, const int *perm, const float *g_loss, const float *g_value, float *g_est,
                                   float *g_target, void *stream) {
    const int rc = check_geometry("sep_metric_bwd", B, S, T, kind, zero_mean, eps);
    if (rc != PSND_OK) return rc;
    if (B == 0 || T == 0) return PSND_OK;
    if (!est || !target || !stats || !perm || !g_est || (!g_loss && !g_value)) PSND_FAIL(PSND_E_ARG, "sep_metric_bwd: null pointer");
    const long long chunks = n_chunks(T);
    if (B * S > 0x7fffffff / chunks)
        PSND_FAIL(PSND_E_SHAPE, "sep_metric_bwd: B=%lld S=%lld T=%lld is more than 2^31 - 1 workgroups", (long long)B, (long long)S, (long long)T);
    hipLaunchKernelGGL(sep_bwd_kernel, dim3((unsigned)(B * S * chunks)), dim3(LANES), 0, static_cast<hipStream_t>(stream), est, target, (int)S,
                       (long long)T, (int)chunks, kind, zero_mean, eps, stats, perm, g_loss, g_value, 1.0 / ((double)B * (double)S), g_est, g_target);
    PSND_CHECK_LAUNCH("sep_metric_bwd");
    return PSND_OK;
}

extern "C" int psnd_snr_gain(const float *x, const float *z, int64_t R, int64_t T, const int64_t *lengths, const float *snr, int64_t snr_n,
                             void *scratch, float *gain, void *stream) {
    if (R < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "snr_gain: R=%lld T=%lld", (long long)R, (long long)T);
    if (snr_n != 1 && snr_n != R) PSND_FAIL(PSND_E_ARG, "snr_gain: snr_n=%lld (1 or R=%lld)", (long long)snr_n, (long long)R);
    if (R == 0) return PSND_OK;
    if (!snr || !gain || (T > 0 && (!x || !z || !scratch))) PSND_FAIL(PSND_E_ARG, "snr_gain: null pointer");
    if ((uintptr_t)scratch % 8) PSND_FAIL(PSND_E_ARG, "snr_gain: scratch must be 8-byte aligned");
    const long long spans = n_spans(T);
    if (spans > 0 && R > 0x7fffffff / spans)
        PSND_FAIL(PSND_E_SHAPE, "snr_gain: R=%lld T=%lld is more than 2^31 - 1 workgroups", (long long)R, (long long)T);
    const long long *len = reinterpret_cast<const long long *>(lengths);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (T > 0) {
        const int rm = launch_moments(x, z, R, 1, T, len, static_cast<double *>(scratch), st);
        if (rm != PSND_OK) return rm;
    }
    hipLaunchKernelGGL(snr_gain_kernel, dim3((unsigned)((R + LANES - 1) / LANES)), dim3(LANES), 0, st, (long long)R, (long long)T, len, (int)spans,
                       (const double *)scratch, snr, (int)(snr_n == R && R > 1), gain);
    PSND_CHECK_LAUNCH("snr_gain");
    return PSND_OK;
}

extern "C" int psnd_mix_rows(const float *x, const float *z, int64_t R, int64_t T, const int64_t *lengths, const float *gain, float *y,
                             void *stream) {
    if (R < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "mix_rows: R=%lld T=%lld", (long long)R, (long long)T);
    if (R == 0 || T == 0) return PSND_OK;
    if (!x || !z || !y || !gain) PSND_FAIL(PSND_E_ARG, "mix_rows: null pointer");
    const long long chunks = n_chunks(T);
    if (R > 0x7fffffff / chunks)
        PSND_FAIL(PSND_E_SHAPE, "mix_rows: R=%lld T=%lld is more than 2^31 - 1 workgroups", (long long)R, (long long)T);
    hipLaunchKernelGGL(mix_rows_kernel, dim3((unsigned)(R * chunks)), dim3(LANES), 0, static_cast<hipStream_t>(stream), x, z, (long long)T,
                       reinterpret_cast<const long long *>(lengths), (int)chunks, gain, y);
    PSND_CHECK_LAUNCH("mix_rows");
    return PSND_OK;
}
