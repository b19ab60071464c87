// psnd_stft_mr.hip - mixed-radix STFT: forward, backward and inverse for n_fft = 2^a 3^b 5^c that is no power of two
// (400, 480, 600, 800, 960, 1200, 2400, 4000 ...: the torch.stft-convention front ends at speech sample rates).
//
// One complex n-point FFT lives in LDS as two float arrays (re[n], im[n], 8n bytes, 32 KB at n = 4096).  A pass of radix R is
// Stockham's autosort step: butterfly j < n / R reads points j + r n / R, twiddles them by e^{-2 pi i r (j mod Ns) / (Ns R)} (Ns = product
// of the radices before it), takes the R-point DFT in registers and - after a barrier, every thread holding all of its butterflies -
// writes result q to (j - j mod Ns) R + j mod Ns + q Ns of the SAME buffer; the output of the last pass is in natural order.  The
// inverse direction is the same routine with the two arrays swapped (FFT of (im, re) = swapped unnormalised inverse of (re, im)).
//
// Radix order (mr_radices, recorded in the plan header): every 5, every 3, every 4, then one 2 if a factor two is left.  The odd radices
// come first because the scattered write of a pass strides lanes by R while Ns = 1 (odd R: all 32 banks of a half wave; R = 4: four lanes
// per bank); once Ns is a product of odd factors the radix-4 passes write runs of Ns consecutive floats.
//
// Two real frames ride in one transform (frame A in re, frame B in im) and come apart by Hermitian symmetry:
//   X_A[k] = (Z[k] + conj Z[n-k]) / 2,  X_B[k] = (Z[k] - conj Z[n-k]) / 2i;  an odd last frame is paired with zeros.
// The adjoint / inverse packs the other way: H[k] = G_A[k] + i G_B[k] with each G made Hermitian over all n bins, so that the
// unnormalised inverse transform is (y_A, y_B), both real.
//
// Overlap-add is two launches and no float atomic: the frame kernel writes window * y_f to a caller-provided scratch (N, F, n), the gather
// kernel sums for every output sample the frames that cover it - first the sample itself, then its left mirror image, then its right one
// (the fold-back of the reflect padding), frames ascending - so the result is bit-reproducible.
#include "psnd_common.h"
#include <math.h>
#include <string.h>

namespace {

constexpr int kMrMagic = 0x3152464d;   // "MFR1"
constexpr int kMrHeader = 16;          // 4-byte words: magic, n, number of passes, radix[13]
constexpr int kMrMaxPass = 13;
constexpr int kMrMinN = 16, kMrMaxN = 4096;
constexpr int kMrThreads = 256;
constexpr int kMrTile = 8;             // consecutive frames per workgroup (even: pairs never straddle two workgroups)

bool mr_covered(int n) {
    if (n < kMrMinN || n > kMrMaxN || (n & 1) || (n & (n - 1)) == 0) return false;
    for (int p : {2, 3, 5})
        while (n % p == 0) n /= p;
    return n == 1;
}

// radices of the passes in execution order; returns their count
int mr_radices(int n, int *r) {
    int c = 0;
    while (n % 5 == 0) r[c++] = 5, n /= 5;
    while (n % 3 == 0) r[c++] = 3, n /= 3;
    while (n % 4 == 0) r[c++] = 4, n /= 4;
    if (n == 2) r[c++] = 2;
    return c;
}

struct MrParams {
    const float *wav;
    const float *plan;
    float *mag, *phase, *re, *im;        // forward outputs (any subset)
    const float *gmag, *gre, *gim;       // backward sources; inverse: gmag = magnitude, gre = phase; on (re, im): gmag = re, gre = im, gim = mask
    float *scratch;                      // (N, F, n) windowed frames of the backward / inverse
    long long T, F;
    int n, hop, pad;
    float mag_eps, inv_n;
    int mask_kind;                       // PSND_MASK_* of the inverse on (re, im)
    int npass;
    int radix[kMrMaxPass];
};

// ---------------------------------------------------------------------------------------------
// R-point DFT, forward sign, in place
// ---------------------------------------------------------------------------------------------
template <int R>
__host__ __device__ __forceinline__ void mr_dft(float (&xr)[R], float (&xi)[R]) {
    if constexpr (R == 2) {
        const float ar = xr[0], ai = xi[0];
        xr[0] = ar + xr[1], xi[0] = ai + xi[1];
        xr[1] = ar - xr[1], xi[1] = ai - xi[1];
    } else if constexpr (R == 3) {
        constexpr float s = 0.86602540378443864676f;
        const float tr = xr[1] + xr[2], ti = xi[1] + xi[2];
        const float ur = xr[0] - 0.5f * tr, ui = xi[0] - 0.5f * ti;
        const float dr = (xr[1] - xr[2]) * s, di = (xi[1] - xi[2]) * s;
        xr[0] += tr, xi[0] += ti;
        xr[1] = ur + di, xi[1] = ui - dr;      // u - i d
        xr[2] = ur - di, xi[2] = ui + dr;      // u + i d
    } else if constexpr (R == 4) {
        const float ar = xr[0] + xr[2], ai = xi[0] + xi[2];
        const float br = xr[0] - xr[2], bi = xi[0] - xi[2];
        const float cr = xr[1] + xr[3], ci = xi[1] + xi[3];
        const float dr = xr[1] - xr[3], di = xi[1] - xi[3];
        xr[0] = ar + cr, xi[0] = ai + ci;
        xr[2] = ar - cr, xi[2] = ai - ci;
        xr[1] = br + di, xi[1] = bi - dr;      // b - i d
        xr[3] = br - di, xi[3] = bi + dr;      // b + i d
    } else {
        static_assert(R == 5, "radix");
        constexpr float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f;
        constexpr float s1 = 0.95105651629515357212f, s2 = 0.58778525229247312917f;
        const float a1r = xr[1] + xr[4], a1i = xi[1] + xi[4], b1r = xr[1] - xr[4], b1i = xi[1] - xi[4];
        const float a2r = xr[2] + xr[3], a2i = xi[2] + xi[3], b2r = xr[2] - xr[3], b2i = xi[2] - xi[3];
        const float p1r = xr[0] + c1 * a1r + c2 * a2r, p1i = xi[0] + c1 * a1i + c2 * a2i;
        const float p2r = xr[0] + c2 * a1r + c1 * a2r, p2i = xi[0] + c2 * a1i + c1 * a2i;
        const float q1r = s1 * b1r + s2 * b2r, q1i = s1 * b1i + s2 * b2i;
        const float q2r = s2 * b1r - s1 * b2r, q2i = s2 * b1i - s1 * b2i;
        xr[0] += a1r + a2r, xi[0] += a1i + a2i;
        xr[1] = p1r + q1i, xi[1] = p1i - q1r;  // p1 - i q1
        xr[4] = p1r - q1i, xi[4] = p1i + q1r;
        xr[2] = p2r + q2i, xi[2] = p2i - q2r;  // p2 - i q2
        xr[3] = p2r - q2i, xi[3] = p2i + q2r;
    }
}

// the butterflies one thread holds across the barrier of a pass
template <int R>
struct MrRegs {
    static constexpr int B = (kMrMaxN / R + kMrThreads - 1) / kMrThreads;
    float r[B][R], i[B][R];
};

// tw[j] = (cos, -sin)(2 pi j / n) as consecutive floats
template <int R>
__host__ __device__ __forceinline__ void mr_pass_load(const float *a, const float *b, int n, int Ns, const float *tw, int tid, MrRegs<R> &v) {
    const int nb = n / R, tstep = nb / Ns;
#pragma unroll
    for (int u = 0; u < MrRegs<R>::B; ++u) {
        const int j = tid + kMrThreads * u;
        if (j < nb) {
            const int k = j % Ns;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float x = a[j + r * nb], y = b[j + r * nb];
                if (r == 0) {
                    v.r[u][r] = x, v.i[u][r] = y;
                } else {
                    const int ti = 2 * (r * k * tstep);          // r k tstep < n
                    const float c = tw[ti], s = tw[ti + 1];
                    v.r[u][r] = x * c - y * s;
                    v.i[u][r] = x * s + y * c;
                }
            }
            mr_dft<R>(v.r[u], v.i[u]);
        }
    }
}

template <int R>
__host__ __device__ __forceinline__ void mr_pass_store(float *a, float *b, int n, int Ns, int tid, const MrRegs<R> &v) {
    const int nb = n / R;
#pragma unroll
    for (int u = 0; u < MrRegs<R>::B; ++u) {
        const int j = tid + kMrThreads * u;
        if (j < nb) {
            const int k = j % Ns;
            const int j0 = (j - k) * R + k;                       // j0 + (R - 1) Ns < n
#pragma unroll
            for (int q = 0; q < R; ++q) a[j0 + q * Ns] = v.r[u][q], b[j0 + q * Ns] = v.i[u][q];
        }
    }
}

template <int R>
__device__ __forceinline__ void mr_pass(float *a, float *b, int n, int Ns, const float *tw, int tid) {
    MrRegs<R> v;
    mr_pass_load<R>(a, b, n, Ns, tw, tid, v);
    __syncthreads();
    mr_pass_store<R>(a, b, n, Ns, tid, v);
    __syncthreads();
}

// forward FFT of (a + i b), natural order in and out; call with (b, a) for the unnormalised inverse.  The caller has a barrier between
// its writes to the buffer and this call; the routine ends on a barrier.
__device__ __forceinline__ void mr_fft(float *a, float *b, const MrParams &p, const float *tw, int tid) {
    int Ns = 1;
    for (int s = 0; s < p.npass; ++s) {
        const int R = p.radix[s];
        if (R == 5) mr_pass<5>(a, b, p.n, Ns, tw, tid);
        else if (R == 3) mr_pass<3>(a, b, p.n, Ns, tw, tid);
        else if (R == 4) mr_pass<4>(a, b, p.n, Ns, tw, tid);
        else mr_pass<2>(a, b, p.n, Ns, tw, tid);
        Ns *= R;
    }
}

// windowed frames f (-> re) and f + 1 (-> im, zeros when has_b is false); the reflect padding is index arithmetic
__device__ __forceinline__ void mr_load_pair(float *sre, float *sim, const MrParams &p, const float *x, const float *win, long long f, bool has_b,
                                             int tid) {
    const long long s0 = f * p.hop - p.pad;
    for (int m = tid; m < p.n; m += kMrThreads) {
        const float w = win[m];
        sre[m] = x[reflect_idx(s0 + m, p.T)] * w;
        sim[m] = has_b ? x[reflect_idx(s0 + p.hop + m, p.T)] * w : 0.f;
    }
}

// spectra of the two packed frames at bin k <= n / 2 from Z[k] and Z[n - k]
__device__ __forceinline__ void mr_split(const float *sre, const float *sim, int n, int k, float &ar, float &ai, float &br, float &bi) {
    const int kc = k == 0 ? 0 : n - k;
    const float zr = sre[k], zi = sim[k], cr = sre[kc], ci = sim[kc];
    ar = 0.5f * (zr + cr), ai = 0.5f * (zi - ci);
    br = 0.5f * (zi + ci), bi = 0.5f * (cr - zr);
}

// ---------------------------------------------------------------------------------------------
// forward: grid (ceil(F / kMrTile), N); outputs (N, K, F), two consecutive frames per bin and transform
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMrThreads) void stft_mr_fwd_kernel(MrParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sre = smem, *sim = smem + p.n;
    const int tid = threadIdx.x, n = p.n, half = n / 2;
    const long long clip = blockIdx.y;
    const float *x = p.wav + (size_t)clip * (size_t)p.T;
    const float *win = p.plan + kMrHeader, *tw = win + n;
    const long long f0 = (long long)blockIdx.x * kMrTile;
    const long long f1 = f0 + kMrTile < p.F ? f0 + kMrTile : p.F;
    const size_t cbase = (size_t)clip * (size_t)(half + 1) * (size_t)p.F;
    for (long long f = f0; f < f1; f += 2) {
        const bool has_b = f + 1 < p.F;
        mr_load_pair(sre, sim, p, x, win, f, has_b, tid);
        __syncthreads();
        mr_fft(sre, sim, p, tw, tid);
        for (int k = tid; k <= half; k += kMrThreads) {
            float ar, ai, br, bi;
            mr_split(sre, sim, n, k, ar, ai, br, bi);
            const size_t o = cbase + (size_t)k * (size_t)p.F + (size_t)f;
            if (p.mag) {
                p.mag[o] = __builtin_sqrtf(ar * ar + ai * ai + p.mag_eps);
                if (has_b) p.mag[o + 1] = __builtin_sqrtf(br * br + bi * bi + p.mag_eps);
            }
            if (p.phase) {
                p.phase[o] = atan2f(ai, ar);
                if (has_b) p.phase[o + 1] = atan2f(bi, br);
            }
            if (p.re) {
                p.re[o] = ar, p.im[o] = ai;
                if (has_b) p.re[o + 1] = br, p.im[o + 1] = bi;
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// backward / inverse, launch 1: window * (adjoint or inverse real DFT) of every frame -> scratch (N, F, n)
// ---------------------------------------------------------------------------------------------
enum { MR_FROM_MAG = 1, MR_FROM_REIM = 2, MR_ISTFT = 4, MR_ISTFT_REIM = 8 };   // MR_ISTFT_REIM rides on MR_ISTFT: the (re, im) loader

template <int MODE>
__global__ __launch_bounds__(kMrThreads) void stft_mr_frames_kernel(MrParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float *sre = smem, *sim = smem + p.n;
    const int tid = threadIdx.x, n = p.n, half = n / 2;
    const long long clip = blockIdx.y;
    const float *win = p.plan + kMrHeader, *tw = win + n;
    const long long f0 = (long long)blockIdx.x * kMrTile;
    const long long f1 = f0 + kMrTile < p.F ? f0 + kMrTile : p.F;
    const size_t cbase = (size_t)clip * (size_t)(half + 1) * (size_t)p.F;
    float *sc = p.scratch + (size_t)clip * (size_t)p.F * (size_t)n;
    for (long long f = f0; f < f1; f += 2) {
        const bool has_b = f + 1 < p.F;
        if constexpr ((MODE & MR_FROM_MAG) != 0) {       // recompute X of both frames
            mr_load_pair(sre, sim, p, p.wav + (size_t)clip * (size_t)p.T, win, f, has_b, tid);
            __syncthreads();
            mr_fft(sre, sim, p, tw, tid);
        }
        // bin k and its mirror n - k belong to one thread: it reads Z there (FROM_MAG) and writes H there, no barrier in between
        for (int k = tid; k <= half; k += kMrThreads) {
            const size_t o = cbase + (size_t)k * (size_t)p.F + (size_t)f;
            float gar = 0.f, gai = 0.f, gbr = 0.f, gbi = 0.f;
            if constexpr ((MODE & MR_FROM_MAG) != 0) {
                float ar, ai, br, bi;
                mr_split(sre, sim, n, k, ar, ai, br, bi);
                const float ga = p.gmag[o] / __builtin_sqrtf(ar * ar + ai * ai + p.mag_eps);    // 0 / 0 = NaN as autograd of sqrt
                gar = ga * ar, gai = ga * ai;
                if (has_b) {
                    const float gb = p.gmag[o + 1] / __builtin_sqrtf(br * br + bi * bi + p.mag_eps);
                    gbr = gb * br, gbi = gb * bi;
                }
            }
            if constexpr ((MODE & MR_FROM_REIM) != 0) {
                gar += p.gre[o], gai += p.gim[o];
                if (has_b) gbr += p.gre[o + 1], gbi += p.gim[o + 1];
            }
            if constexpr ((MODE & MR_ISTFT_REIM) != 0) {  // X = m (re + i im), scaled as below
                const float ma = reim_mask(p.mask_kind, p.gim ? p.gim[o] : 1.f) * p.inv_n;
                gar = ma * p.gmag[o], gai = ma * p.gre[o];
                if (has_b) {
                    const float mb = reim_mask(p.mask_kind, p.gim ? p.gim[o + 1] : 1.f) * p.inv_n;
                    gbr = mb * p.gmag[o + 1], gbi = mb * p.gre[o + 1];
                }
            } else if constexpr ((MODE & MR_ISTFT) != 0) {      // X / n; the Hermitian extension below supplies the factor two of the interior bins
                float sn, cs;
                sincosf(p.gre[o], &sn, &cs);
                const float ma = p.gmag[o] * p.inv_n;
                gar = ma * cs, gai = ma * sn;
                if (has_b) {
                    sincosf(p.gre[o + 1], &sn, &cs);
                    const float mb = p.gmag[o + 1] * p.inv_n;
                    gbr = mb * cs, gbi = mb * sn;
                }
            }
            if (k == 0 || k == half) {                   // the imaginary parts of DC and Nyquist do not reach the signal
                sre[k] = gar, sim[k] = gbr;
            } else {
                const float s = (MODE & MR_ISTFT) ? 1.f : 0.5f;
                sre[k] = s * (gar - gbi), sim[k] = s * (gai + gbr);              // G_A + i G_B
                sre[n - k] = s * (gar + gbi), sim[n - k] = s * (gbr - gai);      // conj G_A + i conj G_B
            }
        }
        __syncthreads();
        mr_fft(sim, sre, p, tw, tid);                    // unnormalised inverse: sre = y_A, sim = y_B
        float *ya = sc + (size_t)f * (size_t)n;
        for (int m = tid; m < n; m += kMrThreads) {
            const float w = win[m];
            ya[m] = w * sre[m];
            if (has_b) ya[n + m] = w * sim[m];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// backward / inverse, launch 2: every output sample gathers its frames in a fixed order.
//   backward: out (N, T), sample t receives the taps that read t, -t or 2 (T - 1) - t (reflect padding), pad as the forward's
//   inverse:  out (N, (F - 1) hop), sample t is position t + n / 2 of the overlap-add, divided by the squared-window envelope + eps
// ---------------------------------------------------------------------------------------------
template <bool ISTFT>
__global__ __launch_bounds__(kMrThreads) void stft_mr_gather_kernel(const float *scratch, const float *win, float *out, long long T, long long F, int n,
                                                                    int hop, int pad, float eps) {
    const long long t = (long long)blockIdx.x * kMrThreads + threadIdx.x;
    if (t >= T) return;
    const long long clip = blockIdx.y;
    const float *sc = scratch + (size_t)clip * (size_t)F * (size_t)n;
    float acc = 0.f, env = 0.f;
    auto add = [&](long long u) {                         // u: index into the unpadded signal before reflection, u + pad >= 0
        const long long pp = u + pad;
        long long fhi = pp / hop;
        if (fhi > F - 1) fhi = F - 1;
        const long long flo = pp - n + 1 <= 0 ? 0 : (pp - n + hop) / hop;
        for (long long f = flo; f <= fhi; ++f) {
            const int m = (int)(pp - f * hop);           // 0 <= m < n by the bounds of f
            acc += sc[(size_t)f * (size_t)n + (size_t)m];
            if (ISTFT) env += win[m] * win[m];
        }
    };
    add(t);
    if (!ISTFT) {
        if (t >= 1 && t <= pad) add(-t);
        if (t <= T - 2) add(2 * (T - 1) - t);
    }
    out[(size_t)clip * (size_t)T + (size_t)t] = ISTFT ? acc / (env + eps) : acc;
}

int mr_pad(int n_fft, int hop, int framing) {
    return framing == PSND_FRAMING_NONE ? 0 : (framing == PSND_FRAMING_CENTER ? n_fft / 2 : (n_fft - hop) / 2);
}

void mr_fill(MrParams &p, int n_fft, const void *plan) {
    memset(&p, 0, sizeof(p));
    p.plan = static_cast<const float *>(plan);
    p.n = n_fft;
    p.npass = mr_radices(n_fft, p.radix);
    p.inv_n = 1.0f / (float)n_fft;
}

}  // namespace

const float *psnd_stft_mr_plan_window(const void *plan) { return static_cast<const float *>(plan) + kMrHeader; }

extern "C" size_t psnd_stft_mr_plan_bytes(int n_fft) {
    return mr_covered(n_fft) ? sizeof(float) * (size_t)(kMrHeader + 3 * n_fft) : 0;
}

extern "C" int psnd_stft_mr_plan_build(int n_fft, const float *window_host, void *plan_host) {
    if (!window_host || !plan_host) PSND_FAIL(PSND_E_ARG, "stft_mr_plan_build: null pointer");
    if (!mr_covered(n_fft))
        PSND_FAIL(PSND_E_UNSUPPORTED, "stft_mr_plan_build: n_fft=%d unsupported (even 2^a 3^b 5^c in [16,4096], no power of two)", n_fft);
    int32_t *hd = static_cast<int32_t *>(plan_host);
    memset(hd, 0, sizeof(int32_t) * kMrHeader);
    int radix[kMrMaxPass];
    const int np = mr_radices(n_fft, radix);
    hd[0] = kMrMagic, hd[1] = n_fft, hd[2] = np;
    for (int i = 0; i < np; ++i) hd[3 + i] = radix[i];
    float *win = static_cast<float *>(plan_host) + kMrHeader, *tw = win + n_fft;
    memcpy(win, window_host, sizeof(float) * (size_t)n_fft);
    const double two_pi = 6.283185307179586476925286766559;
    for (int j = 0; j < n_fft; ++j) {
        const double th = two_pi * (double)j / (double)n_fft;
        tw[2 * j] = (float)cos(th);
        tw[2 * j + 1] = (float)(-sin(th));
    }
    return PSND_OK;
}

// checks shared by the three transforms; 1: nothing to do, 0: go on, < 0: error
static int mr_check(const char *what, int64_t N, int64_t T, int64_t F, int n_fft, size_t plan_bytes) {
    if (!mr_covered(n_fft)) PSND_FAIL(PSND_E_UNSUPPORTED, "%s: n_fft=%d unsupported (even 2^a 3^b 5^c in [16,4096], no power of two)", what, n_fft);
    if (plan_bytes != psnd_stft_mr_plan_bytes(n_fft))
        PSND_FAIL(PSND_E_ARG, "%s: a plan of %zu bytes is not the mixed-radix plan of n_fft=%d (%zu bytes)", what, plan_bytes, n_fft,
                  psnd_stft_mr_plan_bytes(n_fft));
    if (T >= ((int64_t)1 << 31) - 4 * (int64_t)n_fft) PSND_FAIL(PSND_E_SHAPE, "%s: T=%lld exceeds 2^31 samples per clip", what, (long long)T);
    if ((int64_t)(n_fft / 2 + 1) * F >= (int64_t)1 << 31) PSND_FAIL(PSND_E_SHAPE, "%s: K*F exceeds 2^31 per clip", what);
    if (N > 65535) PSND_FAIL(PSND_E_SHAPE, "%s: N=%lld exceeds 65535 clips", what, (long long)N);
    return PSND_OK;
}

extern "C" int psnd_stft_mr_fwd(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing, const void *plan, size_t plan_bytes,
                                float mag_eps, float *mag, float *phase, float *re, float *im, void *stream) {
    if (!wav || !plan) PSND_FAIL(PSND_E_ARG, "stft_mr_fwd: null wav/plan");
    if ((re == nullptr) != (im == nullptr)) PSND_FAIL(PSND_E_ARG, "stft_mr_fwd: re and im must be given together");
    if (!mag && !phase && !re) PSND_FAIL(PSND_E_ARG, "stft_mr_fwd: no output requested");
    if (framing < PSND_FRAMING_CENTER || framing > PSND_FRAMING_NONE) PSND_FAIL(PSND_E_ARG, "stft_mr_fwd: framing=%d", framing);
    if (hop <= 0 || N < 0) PSND_FAIL(PSND_E_ARG, "stft_mr_fwd: hop=%d N=%lld", hop, (long long)N);
    const int pad = mr_pad(n_fft, hop, framing);
    const int64_t F = pad < 0 ? 0 : psnd_frame_count(T, n_fft, hop, framing);
    const int rc = mr_check("stft_mr_fwd", N, T, F, n_fft, plan_bytes);
    if (rc != PSND_OK) return rc;
    if (pad < 0 || T <= pad) PSND_FAIL(PSND_E_SHAPE, "stft_mr_fwd: reflect padding %d needs T > pad (T=%lld)", pad, (long long)T);
    if (N == 0 || F <= 0) return PSND_OK;
    MrParams p;
    mr_fill(p, n_fft, plan);
    p.wav = wav, p.mag = mag, p.phase = phase, p.re = re, p.im = im;
    p.T = T, p.F = F, p.hop = hop, p.pad = pad, p.mag_eps = mag_eps;
    const dim3 grid((unsigned)((F + kMrTile - 1) / kMrTile), (unsigned)N);
    hipLaunchKernelGGL(stft_mr_fwd_kernel, grid, dim3(kMrThreads), sizeof(float) * 2 * (size_t)n_fft, static_cast<hipStream_t>(stream), p);
    PSND_CHECK_LAUNCH("stft_mr_fwd");
    return PSND_OK;
}

extern "C" size_t psnd_stft_mr_bwd_scratch_bytes(int64_t N, int64_t T, int n_fft, int hop, int framing) {
    if (!mr_covered(n_fft) || hop <= 0 || N <= 0 || framing < PSND_FRAMING_CENTER || framing > PSND_FRAMING_NONE) return 0;
    if (mr_pad(n_fft, hop, framing) < 0) return 0;
    const int64_t F = psnd_frame_count(T, n_fft, hop, framing);
    return F <= 0 ? 0 : sizeof(float) * (size_t)N * (size_t)F * (size_t)n_fft;
}

extern "C" int psnd_stft_mr_bwd(const float *wav, int64_t N, int64_t T, int n_fft, int hop, int framing, const void *plan, size_t plan_bytes,
                                float mag_eps, const float *gmag, const float *gre, const float *gim, void *scratch, size_t scratch_bytes,
                                float *gwav, void *stream) {
    if (!plan || !gwav) PSND_FAIL(PSND_E_ARG, "stft_mr_bwd: null plan/gwav");
    if ((gre == nullptr) != (gim == nullptr)) PSND_FAIL(PSND_E_ARG, "stft_mr_bwd: gre and gim must be given together");
    if (!gmag && !gre) PSND_FAIL(PSND_E_ARG, "stft_mr_bwd: no gradient source");
    if (gmag && !wav) PSND_FAIL(PSND_E_ARG, "stft_mr_bwd: gmag needs wav (recompute)");
    if (framing < PSND_FRAMING_CENTER || framing > PSND_FRAMING_NONE) PSND_FAIL(PSND_E_ARG, "stft_mr_bwd: framing=%d", framing);
    if (hop <= 0 || N < 0) PSND_FAIL(PSND_E_ARG, "stft_mr_bwd: hop=%d N=%lld", hop, (long long)N);
    const int pad = mr_pad(n_fft, hop, framing);
    const int64_t F = pad < 0 ? 0 : psnd_frame_count(T, n_fft, hop, framing);
    const int rc = mr_check("stft_mr_bwd", N, T, F, n_fft, plan_bytes);
    if (rc != PSND_OK) return rc;
    if (pad < 0 || T <= pad) PSND_FAIL(PSND_E_SHAPE, "stft_mr_bwd: reflect padding %d needs T > pad (T=%lld)", pad, (long long)T);
    if (N == 0) return PSND_OK;
    const size_t need = psnd_stft_mr_bwd_scratch_bytes(N, T, n_fft, hop, framing);
    if (need > 0 && (!scratch || scratch_bytes < need))
        PSND_FAIL(PSND_E_ARG, "stft_mr_bwd: scratch of %zu bytes, psnd_stft_mr_bwd_scratch_bytes asks for %zu", scratch ? scratch_bytes : (size_t)0, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    MrParams p;
    mr_fill(p, n_fft, plan);
    p.wav = wav, p.gmag = gmag, p.gre = gre, p.gim = gim, p.scratch = static_cast<float *>(scratch);
    p.T = T, p.F = F, p.hop = hop, p.pad = pad, p.mag_eps = mag_eps;
    if (F > 0) {
        const dim3 grid((unsigned)((F + kMrTile - 1) / kMrTile), (unsigned)N);
        const size_t lds = sizeof(float) * 2 * (size_t)n_fft;
        if (gmag && !gre) hipLaunchKernelGGL((stft_mr_frames_kernel<MR_FROM_MAG>), grid, dim3(kMrThreads), lds, s, p);
        else if (!gmag) hipLaunchKernelGGL((stft_mr_frames_kernel<MR_FROM_REIM>), grid, dim3(kMrThreads), lds, s, p);
        else hipLaunchKernelGGL((stft_mr_frames_kernel<MR_FROM_MAG | MR_FROM_REIM>), grid, dim3(kMrThreads), lds, s, p);
        PSND_CHECK_LAUNCH("stft_mr_bwd(frames)");
    }
    // F = 0: the gather finds no frame and writes zeros
    const dim3 ggrid((unsigned)((T + kMrThreads - 1) / kMrThreads), (unsigned)N);
    hipLaunchKernelGGL((stft_mr_gather_kernel<false>), ggrid, dim3(kMrThreads), 0, s, p.scratch, p.plan + kMrHeader, gwav, (long long)T, (long long)F,
                       n_fft, hop, pad, 0.f);
    PSND_CHECK_LAUNCH("stft_mr_bwd(gather)");
    return PSND_OK;
}

extern "C" size_t psnd_istft_mr_scratch_bytes(int64_t N, int64_t F, int n_fft) {
    if (!mr_covered(n_fft) || N <= 0 || F <= 1) return 0;
    return sizeof(float) * (size_t)N * (size_t)F * (size_t)n_fft;
}

// REIM: (a, b) = (re, im) with an optional mask instead of (magnitude, phase) - psnd_istft_reim_mr
template <bool REIM>
static int istft_mr_impl(const char *what, const float *a, const float *b, const float *mask, int mask_kind, int64_t N, int64_t F, int n_fft, int hop,
                         const void *plan, size_t plan_bytes, float eps, void *scratch, size_t scratch_bytes, float *out, void *stream) {
    if (!a || !b || !plan || !out) PSND_FAIL(PSND_E_ARG, "%s: null pointer", what);
    if (REIM && (mask_kind < PSND_MASK_NONE || mask_kind > PSND_MASK_SIGMOID || (mask != nullptr) != (mask_kind != PSND_MASK_NONE)))
        PSND_FAIL(PSND_E_ARG, "%s: mask_kind=%d with a %s mask", what, mask_kind, mask ? "non-NULL" : "NULL");
    if (hop <= 0 || N < 0 || F < 0) PSND_FAIL(PSND_E_ARG, "%s: hop=%d N=%lld F=%lld", what, hop, (long long)N, (long long)F);
    const int64_t T = F > 0 ? (F - 1) * hop : 0;
    const int rc = mr_check(what, N, T, F, n_fft, plan_bytes);
    if (rc != PSND_OK) return rc;
    if (N == 0 || F <= 1) return PSND_OK;
    const size_t need = psnd_istft_mr_scratch_bytes(N, F, n_fft);
    if (!scratch || scratch_bytes < need)
        PSND_FAIL(PSND_E_ARG, "%s: scratch of %zu bytes, psnd_istft_mr_scratch_bytes asks for %zu", what, scratch ? scratch_bytes : (size_t)0, need);
    hipStream_t s = static_cast<hipStream_t>(stream);
    MrParams p;
    mr_fill(p, n_fft, plan);
    p.gmag = a, p.gre = b, p.gim = mask, p.mask_kind = mask_kind, p.scratch = static_cast<float *>(scratch);
    p.T = T, p.F = F, p.hop = hop, p.pad = n_fft / 2;
    const dim3 grid((unsigned)((F + kMrTile - 1) / kMrTile), (unsigned)N);
    hipLaunchKernelGGL((stft_mr_frames_kernel<REIM ? (MR_ISTFT | MR_ISTFT_REIM) : MR_ISTFT>), grid, dim3(kMrThreads), sizeof(float) * 2 * (size_t)n_fft, s, p);
    PSND_CHECK_LAUNCH(REIM ? "istft_reim_mr(frames)" : "istft_mr(frames)");
    const dim3 ggrid((unsigned)((T + kMrThreads - 1) / kMrThreads), (unsigned)N);
    hipLaunchKernelGGL((stft_mr_gather_kernel<true>), ggrid, dim3(kMrThreads), 0, s, p.scratch, p.plan + kMrHeader, out, (long long)T, (long long)F, n_fft,
                       hop, n_fft / 2, eps);
    PSND_CHECK_LAUNCH(REIM ? "istft_reim_mr(gather)" : "istft_mr(gather)");
    return PSND_OK;
}

extern "C" int psnd_istft_mr(const float *mag, const float *phase, int64_t N, int64_t F, int n_fft, int hop, const void *plan, size_t plan_bytes,
                             float eps, void *scratch, size_t scratch_bytes, float *out, void *stream) {
    return istft_mr_impl<false>("istft_mr", mag, phase, nullptr, PSND_MASK_NONE, N, F, n_fft, hop, plan, plan_bytes, eps, scratch, scratch_bytes, out,
                                stream);
}

extern "C" int psnd_istft_reim_mr(const float *re, const float *im, const float *mask, int mask_kind, int64_t N, int64_t F, int n_fft, int hop,
                                  const void *plan, size_t plan_bytes, float eps, void *scratch, size_t scratch_bytes, float *out, void *stream) {
    return istft_mr_impl<true>("istft_reim_mr", re, im, mask, mask_kind, N, F, n_fft, hop, plan, plan_bytes, eps, scratch, scratch_bytes, out, stream);
}
