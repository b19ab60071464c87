// psnd_lstft.hip - LearnableSTFT (pytorch_sound/models/transforms.py:104-203) on the gfx950 matrix cores, exact fp32.
// The reference runs the trainable analysis / synthesis filterbank as F.conv1d / F.conv_transpose1d of a (C, 1, n) basis times the
// window with stride hop.  Its three linear operators are contractions whose "unfolded frames" operand is a STRIDED VIEW of a waveform
// (k-stride 1, frame-stride hop), so none of them needs the (N, n, F) frame tensor in memory:
//   analysis   A: spec[z][c][f] = sum_m B[c][m] w[m] x[z][f hop + m]                       M = c, columns = (z, f), K = m
//   synthesis  S: y[z][q hop + r] = sum_{j, c} B[c][j hop + r] w[j hop + r] g[z][c][q - j]  M = r, columns = (z, q), K = (j, c)
//                 (the transposed convolution in gather / polyphase form: every output sample is written once - no atomics, no zero fill)
//   basis grad G: gB[c][m] = w[m] sum_{z, f} g[z][c][f] x[z][f hop + m]                    M = c, columns = m, K = (z, f) in slabs
// One kernel template serves the three: a (BM x BN x 16) tile loop on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: an fmaf chain) with
// the operand loaders and the epilogue chosen by MODE.  MFMA operand convention as in psnd_attn.hip: lane l holds A[i = l & 31][k = l >> 5]
// and B[k = l >> 5][j = l & 31]; D[i][j]: j = l & 31, i = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
#include "psnd_common.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

enum { LS_ANALYSIS = 0, LS_GRAD = 1, LS_SYNTH = 2 };

struct LstftParams {
    const float *a;              // analysis / synthesis: basis (C, n); grad: g (Z, C, F)
    const float *b;              // analysis / grad: waveform (Z, Lx); synthesis: g (Z, C, F)
    const float *w;              // window (n)
    const float *mult;           // synthesis: per-sample multiplier (Lx) or null
    float *out;                  // analysis: spec (Z, C, F); grad: slabs (S, C, n); synthesis: y (Z, Lx)
    int M, cols, K;              // the GEMM's extents (cols: all batches in analysis / synthesis)
    int C, n, hop, F, Z;
    int Q;                       // synthesis: hop blocks per row of y
    long long Lx;                // row length of the waveform operand / of y
    int zchunk, ksplit, kpart;   // grad: a workgroup sums over zchunk clips x one part of kpart frames into its slab
    int tiles_m;
};

constexpr int LBK = 16;

__device__ __forceinline__ int ls_rho(int s, int half) { return (s & 3) + 8 * (s >> 2) + 4 * half; }

// ---- operand loaders.  Two thread maps over a (BX rows x 16 k) tile, BX / 64 float4 per thread:
//   k-contiguous source  : row = tid / 4 + 64 u, k4 = 4 (tid % 4)                - a float4 along k
//   row-contiguous source: k = tid / (BX / 4) + (1024 / BX) u, x4 = 4 (tid % (BX / 4)) - a float4 along the rows
template <int BX>
struct KContig {
    long long base[BX / 64];     // element offset of the thread's rows at k = 0, < 0: no such row
    __device__ __forceinline__ void fetch(const float *src, long long add, int k0, int kend, int tid, f32x4 (&v)[BX / 64]) const {
        const int k = k0 + 4 * (tid & 3);
#pragma unroll
        for (int u = 0; u < BX / 64; ++u) {
            f32x4 r = {0.f, 0.f, 0.f, 0.f};
            if (base[u] >= 0) {
                const float *p = src + base[u] + add + k;
                if (k + 3 < kend) {
                    r = *reinterpret_cast<const f32x4_u *>(p);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k + e < kend) r[e] = p[e];
                }
            }
            v[u] = r;
        }
    }
    static __device__ __forceinline__ void commit(float *tile, int tid, const f32x4 (&v)[BX / 64]) {
#pragma unroll
        for (int u = 0; u < BX / 64; ++u) {
            const int x = (tid >> 2) + 64 * u, k = 4 * (tid & 3);
#pragma unroll
            for (int e = 0; e < 4; ++e) tile[(k + e) * (BX + 4) + x] = v[u][e];
        }
    }
};
template <int BX>
__device__ __forceinline__ void rowcontig_commit(float *tile, int tid, const f32x4 (&v)[BX / 64]) {
#pragma unroll
    for (int u = 0; u < BX / 64; ++u)
        *reinterpret_cast<f32x4 *>(tile + ((tid / (BX / 4)) + (1024 / BX) * u) * (BX + 4) + 4 * (tid % (BX / 4))) = v[u];
}
// four consecutive elements p[0..3] of which the first `nval` exist
__device__ __forceinline__ f32x4 load4(const float *p, int nval) {
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (nval >= 4) {
        r = *reinterpret_cast<const f32x4_u *>(p);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < nval) r[e] = p[e];
    }
    return r;
}

template <int MODE, int BM, int BN>
__global__ __launch_bounds__(256, 2) void lstft_gemm_kernel(LstftParams p) {
    constexpr int PA = BM + 4, PB = BN + 4, UA = BM / 64, UB = BN / 64, TM = BM / 64, TN = BN / 64;
    __shared__ __attribute__((aligned(16))) float sA[2][LBK * PA], sB[2][LBK * PB];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, kk = lane >> 5;
    const int m0 = (blockIdx.x % p.tiles_m) * BM, n0 = (blockIdx.x / p.tiles_m) * BN;
    // grad: slab blockIdx.y = (clip chunk, frame part)
    const int zc = MODE == LS_GRAD ? blockIdx.y / p.ksplit : 0;
    const int kbeg = MODE == LS_GRAD ? (blockIdx.y - zc * p.ksplit) * p.kpart : 0;
    const int kend = MODE == LS_GRAD ? min(p.K, kbeg + p.kpart) : p.K;
    const int z0 = zc * p.zchunk, z1 = MODE == LS_GRAD ? min(z0 + p.zchunk, p.Z) : 1;
    const int nk = kend > kbeg ? (kend - kbeg + LBK - 1) / LBK : 0;
    const int steps = (z1 - z0) * nk;

    // ---- what of the operand addresses does not change along k
    KContig<BM> ka;              // analysis: basis rows; grad: g rows
    KContig<BN> kb;              // analysis: frame starts in the waveform
    const int rowA = m0 + 4 * (tid % (BM / 4));      // synthesis: the thread's four phases r
    const int colB = n0 + 4 * (tid % (BN / 4));      // grad: four taps; synthesis: four columns (z, q)
    long long sb_off[4];         // synthesis: offset of g[z][0][q] per column, and q (< 0: no such column)
    int sb_q[4];
    if constexpr (MODE != LS_SYNTH) {
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int m = m0 + (tid >> 2) + 64 * u;
            ka.base[u] = m < p.M ? (long long)m * (MODE == LS_ANALYSIS ? p.n : p.F) : -1;
        }
    }
    if constexpr (MODE == LS_ANALYSIS) {
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int c = n0 + (tid >> 2) + 64 * u, z = c / p.F, f = c - z * p.F;
            kb.base[u] = c < p.cols ? z * p.Lx + (long long)f * p.hop : -1;
        }
    }
    if constexpr (MODE == LS_SYNTH) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = colB + e, z = c / p.Q, q = c - z * p.Q;
            sb_q[e] = c < p.cols ? q : -(1 << 30);
            sb_off[e] = (long long)z * p.C * p.F + q;
        }
    }

    f32x4 va[UA], vb[UB];
    auto fetch = [&](int it) __attribute__((always_inline)) {
        const int zi = it / nk, k0 = kbeg + (it - zi * nk) * LBK;
        if constexpr (MODE == LS_ANALYSIS) {
            ka.fetch(p.a, 0, k0, kend, tid, va);
            const int k = k0 + 4 * (tid & 3);
            const f32x4 wv = load4(p.w + k, kend - k);               // the reference multiplies the window into the basis first
#pragma unroll
            for (int u = 0; u < UA; ++u) va[u] *= wv;
            kb.fetch(p.b, 0, k0, kend, tid, vb);
        } else if constexpr (MODE == LS_GRAD) {
            const long long z = z0 + zi;
            ka.fetch(p.a, z * p.C * p.F, k0, kend, tid, va);
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int k = k0 + tid / (BN / 4) + (1024 / BN) * u;
                f32x4 r = {0.f, 0.f, 0.f, 0.f};
                if (k < kend) r = load4(p.b + z * p.Lx + (long long)k * p.hop + colB, p.n - colB);
                vb[u] = r;
            }
        } else {
#pragma unroll
            for (int u = 0; u < UA; ++u) {           // basis taps j hop + r of channel c, windowed
                const int k = k0 + tid / (BM / 4) + (1024 / BM) * u, j = k / p.C, c = k - j * p.C, t = j * p.hop + rowA;
                f32x4 r = {0.f, 0.f, 0.f, 0.f};
                if (k < kend) {
                    const int nval = min(p.hop - rowA, p.n - t);
                    r = load4(p.a + (long long)c * p.n + t, nval) * load4(p.w + t, nval);
                }
                va[u] = r;
            }
#pragma unroll
            for (int u = 0; u < UB; ++u) {           // frames q - j of channel c
                const int k = k0 + tid / (BN / 4) + (1024 / BN) * u, j = k / p.C, c = k - j * p.C;
                f32x4 r = {0.f, 0.f, 0.f, 0.f};
                if (k < kend) {
                    const int f = sb_q[0] - j;
                    if (sb_q[3] == sb_q[0] + 3 && f >= 0 && f + 3 < p.F) {       // four frames of one clip
                        r = *reinterpret_cast<const f32x4_u *>(p.b + sb_off[0] + (long long)c * p.F - j);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int fe = sb_q[e] - j;
                            if (fe >= 0 && fe < p.F) r[e] = p.b[sb_off[e] + (long long)c * p.F - j];
                        }
                    }
                }
                vb[u] = r;
            }
        }
    };
    auto commit = [&](int buf) __attribute__((always_inline)) {
        if constexpr (MODE == LS_SYNTH) rowcontig_commit<BM>(sA[buf], tid, va);
        else KContig<BM>::commit(sA[buf], tid, va);
        if constexpr (MODE == LS_ANALYSIS) KContig<BN>::commit(sB[buf], tid, vb);
        else rowcontig_commit<BN>(sB[buf], tid, vb);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

    // k-tile it + 1 is in flight (registers) while k-tile it is multiplied out of LDS; two LDS buffers, one barrier per k-tile
    if (steps > 0) {
        fetch(0);
        commit(0);
    }
    __syncthreads();
    for (int it = 0; it < steps; ++it) {
        const float *tA = sA[it & 1], *tB = sB[it & 1];
        if (it + 1 < steps) fetch(it + 1);
#pragma unroll
        for (int s = 0; s < LBK / 2; ++s) {
            float fa[TM], fb[TN];
#pragma unroll
            for (int t = 0; t < TM; ++t) fa[t] = tA[(2 * s + kk) * PA + wm * (BM / 2) + t * 32 + li];
#pragma unroll
            for (int u = 0; u < TN; ++u) fb[u] = tB[(2 * s + kk) * PB + wn * (BN / 2) + u * 32 + li];
#pragma unroll
            for (int t = 0; t < TM; ++t)
#pragma unroll
                for (int u = 0; u < TN; ++u) acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[t], fb[u], acc[t][u], 0, 0, 0);
        }
        if (it + 1 < steps) commit((it + 1) & 1);    // the buffer k-tile it - 1 was read from: every wave is past the barrier behind it
        __syncthreads();
    }

    // ---- epilogue
#pragma unroll
    for (int u = 0; u < TN; ++u) {
        const int col = n0 + wn * (BN / 2) + u * 32 + li;
        if (col >= p.cols) continue;
        if constexpr (MODE == LS_SYNTH) {            // four consecutive phases r are four consecutive samples
            const int z = col / p.Q, q = col - z * p.Q;
            const long long s0 = (long long)q * p.hop;
            float *yrow = p.out + z * p.Lx;
#pragma unroll
            for (int t = 0; t < TM; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int m = m0 + wm * (BM / 2) + t * 32 + 8 * g + 4 * kk;
                    const long long s = s0 + m;
                    const int nval = (int)min((long long)(p.M - m), p.Lx - s);
                    f32x4 v = {acc[t][u][4 * g], acc[t][u][4 * g + 1], acc[t][u][4 * g + 2], acc[t][u][4 * g + 3]};
                    if (nval <= 0) continue;
                    if (p.mult) v *= load4(p.mult + s, nval);
                    if (nval >= 4) {
                        *reinterpret_cast<f32x4_u *>(yrow + s) = v;
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (e < nval) yrow[s + e] = v[e];
                    }
                }
        } else {
            float *o;
            long long ld;
            if constexpr (MODE == LS_ANALYSIS) {
                const int z = col / p.F, f = col - z * p.F;
                o = p.out + (long long)z * p.C * p.F + f, ld = p.F;
            } else {
                o = p.out + (long long)blockIdx.y * p.C * p.n + col, ld = p.n;
            }
#pragma unroll
            for (int t = 0; t < TM; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = m0 + wm * (BM / 2) + t * 32 + ls_rho(r, kk);
                    if (m < p.M) o[(long long)m * ld] = acc[t][u][r];
                }
        }
    }
}

// gB[c][m] = w[m] * sum over slabs of part[s][c][m], in a fixed order (bit-reproducible): 64 elements x 4 slab groups per workgroup
__global__ __launch_bounds__(256) void lstft_slab_sum_kernel(const float *part, int slabs, long long total, int n, const float *w, float *out) {
    __shared__ float red[4][64];
    const int e = threadIdx.x & 63, g = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * 64 + e;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    if (i < total) {
        int s = g;
        for (; s + 12 < slabs; s += 16) {
            a0 += part[(long long)s * total + i];
            a1 += part[(long long)(s + 4) * total + i];
            a2 += part[(long long)(s + 8) * total + i];
            a3 += part[(long long)(s + 12) * total + i];
        }
        for (; s < slabs; s += 4) a0 += part[(long long)s * total + i];
    }
    red[g][e] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    if (g == 0 && i < total) out[i] = w[i % n] * ((red[0][e] + red[1][e]) + (red[2][e] + red[3][e]));
}

// mag = sqrt(re^2 + im^2), phase = atan2(im, re) of spec (Z, 2 Kb, F): rows [0, Kb) real, [Kb, 2 Kb) imaginary (the reference's chunk(2, 1))
__global__ __launch_bounds__(256) void lstft_polar_kernel(const float *spec, long long KF, long long total, float *mag, float *phase) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long z = i / KF, r = i - z * KF;
    const float re = spec[z * 2 * KF + r], im = spec[z * 2 * KF + KF + r];
    mag[i] = sqrtf(re * re + im * im);
    phase[i] = atan2f(im, re);
}
// gspec = [gmag re / mag ; gmag im / mag] - at a zero bin (gmag / 0) * 0 = NaN, as autograd of sqrt gives (psnd_stft_bwd.hip does the same)
__global__ __launch_bounds__(256) void lstft_mag_bwd_kernel(const float *spec, const float *mag, const float *gmag, long long KF, long long total,
                                                            float *gspec) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long z = i / KF, r = i - z * KF;
    const float s = gmag[i] / mag[i];
    gspec[z * 2 * KF + r] = s * spec[z * 2 * KF + r];
    gspec[z * 2 * KF + KF + r] = s * spec[z * 2 * KF + KF + r];
}

// tile shape: the work of the slowest compute unit - (BM x BN) per workgroup x the rounds 512 resident workgroups (two per CU) need.
// The operators are small next to the chip (126 frames x 32 clips: 66 tiles of 128 x 128), so the smaller tiles usually win.
void pick_tile(long long M, long long cols, long long z, int *bm, int *bn) {
    long long best = -1;
    for (int i = 0; i < 4; ++i) {
        const int m = i & 2 ? 64 : 128, n = i & 1 ? 64 : 128;
        const long long wgs = ((M + m - 1) / m) * ((cols + n - 1) / n) * z;
        const long long cost = (long long)m * n * ((wgs + 511) / 512);
        if (best < 0 || cost < best) best = cost, *bm = m, *bn = n;
    }
}

template <int MODE>
int launch(LstftParams &p, int slabs, hipStream_t st, const char *what) {
    int bm, bn;
    pick_tile(p.M, p.cols, slabs, &bm, &bn);
    p.tiles_m = (p.M + bm - 1) / bm;
    const long long gx = (long long)p.tiles_m * ((p.cols + bn - 1) / bn);
    if (gx > 0x7fffffff || slabs > 65535) PSND_FAIL(PSND_E_UNSUPPORTED, "%s: grid too large", what);
    const dim3 grid((unsigned)gx, (unsigned)slabs);
    if (bm == 128 && bn == 128) hipLaunchKernelGGL((lstft_gemm_kernel<MODE, 128, 128>), grid, dim3(256), 0, st, p);
    else if (bm == 128) hipLaunchKernelGGL((lstft_gemm_kernel<MODE, 128, 64>), grid, dim3(256), 0, st, p);
    else if (bn == 128) hipLaunchKernelGGL((lstft_gemm_kernel<MODE, 64, 128>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((lstft_gemm_kernel<MODE, 64, 64>), grid, dim3(256), 0, st, p);
    PSND_CHECK_LAUNCH(what);
    return PSND_OK;
}

// basis gradient: clip chunks x frame parts so that ~512 workgroups run; parts of a multiple of 16 frames, at least 64
void grad_split(int64_t N, int C, int n, int64_t F, int64_t *zslabs, int *ksplit, int *kpart) {
    const int64_t tiles = (int64_t)((C + 127) / 128) * ((n + 127) / 128);
    int64_t want = 512 / (tiles > 0 ? tiles : 1);
    if (want < 1) want = 1;
    int64_t zs = want > N ? N : want;
    const int64_t chunk = (N + zs - 1) / zs;
    zs = (N + chunk - 1) / chunk;
    int64_t ks = 1;
    if (zs == N && want > N) {
        ks = (want + N - 1) / N;
        const int64_t cap = F / 64 > 1 ? F / 64 : 1;
        if (ks > cap) ks = cap;
    }
    const int64_t kp = ((F + ks - 1) / ks + 15) / 16 * 16;
    ks = (F + kp - 1) / kp;
    *zslabs = zs, *ksplit = (int)ks, *kpart = (int)kp;
}

int check_geometry(const char *what, int64_t N, int64_t Lx, int C, int n, int hop) {
    if (hop <= 0) PSND_FAIL(PSND_E_ARG, "%s: hop=%d (> 0)", what, hop);
    if (n < 2) PSND_FAIL(PSND_E_ARG, "%s: n=%d taps (>= 2)", what, n);
    if (N < 0 || C <= 0) PSND_FAIL(PSND_E_ARG, "%s: N=%lld C=%d", what, (long long)N, C);
    if (Lx < n) PSND_FAIL(PSND_E_ARG, "%s: a row of %lld samples is shorter than the %d taps", what, (long long)Lx, n);
    return PSND_OK;
}

}  // namespace

extern "C" int psnd_lstft_analysis(const float *x, const float *basis, const float *window, int64_t N, int64_t Lx, int C, int n, int hop,
                                   float *spec, float *mag, float *phase, void *stream) {
    if (int rc = check_geometry("lstft_analysis", N, Lx, C, n, hop)) return rc;
    if (!x || !basis || !window || !spec) PSND_FAIL(PSND_E_ARG, "lstft_analysis: null pointer");
    if ((mag == nullptr) != (phase == nullptr)) PSND_FAIL(PSND_E_ARG, "lstft_analysis: mag and phase come together");
    if (mag && (C & 1)) PSND_FAIL(PSND_E_ARG, "lstft_analysis: C=%d rows do not pair into (re, im) for mag / phase", C);
    const int64_t F = (Lx - n) / hop + 1;
    if (N * F >= ((int64_t)1 << 31) || Lx >= ((int64_t)1 << 40)) PSND_FAIL(PSND_E_UNSUPPORTED, "lstft_analysis: %lld x %lld frames", (long long)N, (long long)F);
    if (N == 0) return PSND_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    LstftParams p = {};
    p.a = basis, p.b = x, p.w = window, p.out = spec;
    p.M = C, p.cols = (int)(N * F), p.K = n;
    p.C = C, p.n = n, p.hop = hop, p.F = (int)F, p.Z = (int)N, p.Lx = Lx;
    p.zchunk = 1, p.ksplit = 1, p.kpart = n;
    if (int rc = launch<LS_ANALYSIS>(p, 1, st, "lstft_analysis")) return rc;
    if (mag) {
        const long long KF = (long long)(C / 2) * F, total = N * KF;
        hipLaunchKernelGGL(lstft_polar_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, spec, KF, total, mag, phase);
        PSND_CHECK_LAUNCH("lstft_analysis(polar)");
    }
    return PSND_OK;
}

extern "C" int psnd_lstft_mag_bwd(const float *spec, const float *mag, const float *gmag, int64_t N, int C, int64_t F, float *gspec,
                                  void *stream) {
    if (!spec || !mag || !gmag || !gspec) PSND_FAIL(PSND_E_ARG, "lstft_mag_bwd: null pointer");
    if (N < 0 || C <= 0 || (C & 1) || F <= 0) PSND_FAIL(PSND_E_ARG, "lstft_mag_bwd: N=%lld C=%d (even) F=%lld", (long long)N, C, (long long)F);
    const long long KF = (long long)(C / 2) * F, total = N * KF;
    if (total >= ((int64_t)1 << 39)) PSND_FAIL(PSND_E_UNSUPPORTED, "lstft_mag_bwd: tensor too large");
    if (total == 0) return PSND_OK;
    hipLaunchKernelGGL(lstft_mag_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), spec, mag, gmag,
                       KF, total, gspec);
    PSND_CHECK_LAUNCH("lstft_mag_bwd");
    return PSND_OK;
}

extern "C" int psnd_lstft_synthesis(const float *g, const float *basis, const float *window, const float *mult, int64_t N, int C, int64_t F,
                                    int n, int hop, int64_t Ly, float *y, void *stream) {
    if (int rc = check_geometry("lstft_synthesis", N, Ly, C, n, hop)) return rc;
    if (!g || !basis || !window || !y) PSND_FAIL(PSND_E_ARG, "lstft_synthesis: null pointer");
    if (F <= 0 || Ly < n + (int64_t)hop * (F - 1))
        PSND_FAIL(PSND_E_ARG, "lstft_synthesis: F=%lld frames give %lld samples, the rows of y have %lld", (long long)F,
                  (long long)(n + (int64_t)hop * (F - 1)), (long long)Ly);
    const int64_t Q = (Ly + hop - 1) / hop, J = (n + hop - 1) / hop;
    if (N * Q >= ((int64_t)1 << 31) || J * C >= ((int64_t)1 << 31) || Ly >= ((int64_t)1 << 40) || N * F * C >= ((int64_t)1 << 40))
        PSND_FAIL(PSND_E_UNSUPPORTED, "lstft_synthesis: %lld x %lld hop blocks, %lld x %d taps", (long long)N, (long long)Q, (long long)J, C);
    if (N == 0) return PSND_OK;
    LstftParams p = {};
    p.a = basis, p.b = g, p.w = window, p.mult = mult, p.out = y;
    p.M = hop, p.cols = (int)(N * Q), p.K = (int)(J * C);
    p.C = C, p.n = n, p.hop = hop, p.F = (int)F, p.Z = (int)N, p.Q = (int)Q, p.Lx = Ly;
    p.zchunk = 1, p.ksplit = 1, p.kpart = p.K;
    return launch<LS_SYNTH>(p, 1, static_cast<hipStream_t>(stream), "lstft_synthesis");
}

extern "C" int64_t psnd_lstft_wgrad_slabs(int64_t N, int C, int n, int64_t F) {
    if (N <= 0 || C <= 0 || n <= 0 || F <= 0) return 0;
    int64_t zs;
    int ks, kp;
    grad_split(N, C, n, F, &zs, &ks, &kp);
    return zs * ks;
}

extern "C" int psnd_lstft_basis_grad(const float *g, const float *x, const float *window, int64_t N, int64_t Lx, int C, int n, int hop,
                                     int64_t F, float *gb_part, float *gb, void *stream) {
    if (int rc = check_geometry("lstft_basis_grad", N, Lx, C, n, hop)) return rc;
    if (!g || !x || !window || !gb_part || !gb) PSND_FAIL(PSND_E_ARG, "lstft_basis_grad: null pointer");
    if (F <= 0 || F > (Lx - n) / hop + 1)
        PSND_FAIL(PSND_E_ARG, "lstft_basis_grad: F=%lld frames, rows of %lld samples hold %lld", (long long)F, (long long)Lx, (long long)((Lx - n) / hop + 1));
    if (F >= ((int64_t)1 << 31) || N >= ((int64_t)1 << 31) || Lx >= ((int64_t)1 << 40) || N * F * C >= ((int64_t)1 << 40))
        PSND_FAIL(PSND_E_UNSUPPORTED, "lstft_basis_grad: %lld x %lld frames", (long long)N, (long long)F);
    if (N == 0) PSND_FAIL(PSND_E_ARG, "lstft_basis_grad: empty batch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t zs;
    int ks, kp;
    grad_split(N, C, n, F, &zs, &ks, &kp);
    const int slabs = (int)(zs * ks);
    LstftParams p = {};
    p.a = g, p.b = x, p.w = window, p.out = gb_part;
    p.M = C, p.cols = n, p.K = (int)F;
    p.C = C, p.n = n, p.hop = hop, p.F = (int)F, p.Z = (int)N, p.Lx = Lx;
    p.zchunk = (int)((N + zs - 1) / zs), p.ksplit = ks, p.kpart = kp;
    if (int rc = launch<LS_GRAD>(p, slabs, st, "lstft_basis_grad")) return rc;
    const long long total = (long long)C * n;
    hipLaunchKernelGGL(lstft_slab_sum_kernel, dim3((unsigned)((total + 63) / 64)), dim3(256), 0, st, gb_part, slabs, total, n, window, gb);
    PSND_CHECK_LAUNCH("lstft_basis_grad(slab sum)");
    return PSND_OK;
}
