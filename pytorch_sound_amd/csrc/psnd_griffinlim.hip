// psnd_griffinlim.hip - the two device pieces of Griffin-Lim on (N, K, F) fp32 spectra on gfx950, by the definition of include/psnd.h:
//   start   X0 = S (cos phi, sin phi), or (S, 0) without a phase
//   step    t = C - alpha P,  X = S (t / (hypot(t) + eps)),  and per chunk the sums of (|C| - S)^2 and S^2 for the convergence measure
// What stands between STFT.transform_complex and STFT.inverse_complex in every iteration of kernels.griffinlim.
//
// Streaming kernels: the step reads five planes and writes two, 28 bytes per element, a dozen flops and two hypotf.  An item is taken as
// one run of M = K F elements; a workgroup of 256 lanes takes one chunk of CHUNK = 2048 consecutive elements of ONE item in PASSES = 2 passes
// of 1024, lane l of pass p the V = 4 elements chunk + 1024 p + 4 l ..: one 16-byte load per plane and pass, all of a lane's loads issued
// before its first result is needed (10 in flight per lane).  The vector types are 4-byte aligned (f32x4_u): a plane may start on any
// 4-byte boundary and M may be odd, the memory pipeline splits what is not 16-byte aligned.  A group goes element by element when it
// crosses the end of the item or, in an item with F_n < F valid frames, when it does not lie inside the valid part of one row; nothing is
// loaded at f >= F_n, (0, 0) is stored there.  An item with F_n = F (or no `frames`) takes no division at all.
//   The sums: a lane adds its elements in ascending order, a wave its lanes by a shuffle tree, lane 0 the four waves in ascending order
//   through 8 floats of LDS - a fixed order, no atomics; one pair per chunk in `partial`.
//   X may be written over P: a lane loads the P elements of both of its passes before it stores anything, and no lane touches another
//   lane's elements.
// Loads and stores are the plain ones: the next kernel of the loop (the inverse transform) reads X right away, and for spectra that fit the
// last-level cache a nontemporal hint would give that up; no variant with the hint has been measured.
#include "psnd_common.h"

namespace {

constexpr int THREADS = 256;
constexpr int V = 4;
constexpr int PASSES = 2;
constexpr unsigned SPAN = THREADS * V;
constexpr unsigned CHUNK = SPAN * PASSES;

__device__ __forceinline__ unsigned valid_frames(const long long *frames, unsigned n, unsigned F) {
    if (!frames) return F;
    const long long v = frames[n];
    return v < 0 ? 0u : (v > (long long)F ? F : (unsigned)v);
}

// one element of the step.  The multiply-add is spelled out so that the vector and the element-by-element road give the same bits.
template <bool HAS_P, bool WANT>
__device__ __forceinline__ void step_elem(float S, float cr, float ci, float pr, float pi, float alpha, float eps, float &xr, float &xi,
                                          float &sum_d, float &sum_s) {
    const float tr = HAS_P ? __builtin_fmaf(-alpha, pr, cr) : cr;
    const float ti = HAS_P ? __builtin_fmaf(-alpha, pi, ci) : ci;
    const float den = hypotf(tr, ti) + eps;
    xr = S * (tr / den);
    xi = S * (ti / den);
    if (WANT) {
        const float d = hypotf(cr, ci) - S;
        sum_d = __builtin_fmaf(d, d, sum_d);
        sum_s = __builtin_fmaf(S, S, sum_s);
    }
}

// how a lane takes its group of V elements at e: 0 nothing (behind the item), 1 as vectors (all inside the item and valid), 2 one by one
__device__ __forceinline__ int group_mode(unsigned e, unsigned M, unsigned F, unsigned Fn, unsigned &f0) {
    f0 = 0;
    if (e >= M) return 0;
    const bool inside = e + V <= M;
    if (Fn >= F) return inside ? 1 : 2;                  // every element of the item is valid: no frame index is needed
    f0 = e % F;
    return inside && f0 + V <= Fn ? 1 : 2;
}

template <bool HAS_P, bool WANT>
__global__ __launch_bounds__(THREADS) void gl_step_kernel(const float *__restrict__ mag, const float *__restrict__ cre,
                                                          const float *__restrict__ cim, const float *pre, const float *pim,
                                                          unsigned chunks, unsigned M, unsigned F, const long long *__restrict__ frames,
                                                          float alpha, float eps, float *xre, float *xim, float *__restrict__ partial) {
    const unsigned n = blockIdx.x / chunks, c = blockIdx.x - n * chunks;
    const unsigned Fn = valid_frames(frames, n, F);
    const size_t off = (size_t)n * M;
    mag += off, cre += off, cim += off, xre += off, xim += off;
    if (HAS_P) pre += off, pim += off;
    int mode[PASSES];
    unsigned f0[PASSES];
    f32x4_u s[PASSES], cr[PASSES], ci[PASSES], pr[PASSES], pi[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const unsigned e = c * CHUNK + p * SPAN + threadIdx.x * V;
        mode[p] = group_mode(e, M, F, Fn, f0[p]);
        pr[p] = pi[p] = f32x4_u{0.f, 0.f, 0.f, 0.f};
        if (mode[p] == 1) {
            s[p] = *reinterpret_cast<const f32x4_u *>(mag + e);
            cr[p] = *reinterpret_cast<const f32x4_u *>(cre + e);
            ci[p] = *reinterpret_cast<const f32x4_u *>(cim + e);
            if (HAS_P) {
                pr[p] = *reinterpret_cast<const f32x4_u *>(pre + e);
                pi[p] = *reinterpret_cast<const f32x4_u *>(pim + e);
            }
        }
    }
    float sum_d = 0.f, sum_s = 0.f;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const unsigned e = c * CHUNK + p * SPAN + threadIdx.x * V;
        if (mode[p] == 1) {
            f32x4_u xr, xi;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float a, b;
                step_elem<HAS_P, WANT>(s[p][v], cr[p][v], ci[p][v], pr[p][v], pi[p][v], alpha, eps, a, b, sum_d, sum_s);
                xr[v] = a, xi[v] = b;
            }
            *reinterpret_cast<f32x4_u *>(xre + e) = xr;
            *reinterpret_cast<f32x4_u *>(xim + e) = xi;
        } else if (mode[p] == 2) {
            for (int v = 0; v < V; ++v) {
                const unsigned ee = e + v;
                if (ee >= M) break;
                float a = 0.f, b = 0.f;
                if (Fn >= F || (f0[p] + v) % F < Fn)
                    step_elem<HAS_P, WANT>(mag[ee], cre[ee], cim[ee], HAS_P ? pre[ee] : 0.f, HAS_P ? pim[ee] : 0.f, alpha, eps, a, b, sum_d,
                                           sum_s);
                xre[ee] = a, xim[ee] = b;
            }
        }
    }
    if (WANT) {
        __shared__ float red[2][THREADS / 64];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            sum_d += __shfl_down(sum_d, o, 64);
            sum_s += __shfl_down(sum_s, o, 64);
        }
        if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = sum_d, red[1][threadIdx.x >> 6] = sum_s;
        __syncthreads();
        if (threadIdx.x == 0) {
            float d = red[0][0], q = red[1][0];
            for (int w = 1; w < THREADS / 64; ++w) d += red[0][w], q += red[1][w];
            float *out = partial + ((size_t)n * chunks + c) * 2;
            out[0] = d, out[1] = q;
        }
    }
}

template <bool HAS_PHI>
__global__ __launch_bounds__(THREADS) void gl_start_kernel(const float *__restrict__ mag, const float *__restrict__ phase, unsigned chunks,
                                                           unsigned M, unsigned F, const long long *__restrict__ frames,
                                                           float *__restrict__ xre, float *__restrict__ xim) {
    const unsigned n = blockIdx.x / chunks, c = blockIdx.x - n * chunks;
    const unsigned Fn = valid_frames(frames, n, F);
    const size_t off = (size_t)n * M;
    mag += off, xre += off, xim += off;
    if (HAS_PHI) phase += off;
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const unsigned e = c * CHUNK + p * SPAN + threadIdx.x * V;
        unsigned f0;
        const int mode = group_mode(e, M, F, Fn, f0);
        if (mode == 1) {
            const f32x4_u s = *reinterpret_cast<const f32x4_u *>(mag + e);
            f32x4_u xr = s, xi = f32x4_u{0.f, 0.f, 0.f, 0.f};
            if (HAS_PHI) {
                const f32x4_u ph = *reinterpret_cast<const f32x4_u *>(phase + e);
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    float sn, cs;
                    sincosf(ph[v], &sn, &cs);
                    xr[v] = s[v] * cs, xi[v] = s[v] * sn;
                }
            }
            *reinterpret_cast<f32x4_u *>(xre + e) = xr;
            *reinterpret_cast<f32x4_u *>(xim + e) = xi;
        } else if (mode == 2) {
            for (int v = 0; v < V; ++v) {
                const unsigned ee = e + v;
                if (ee >= M) break;
                float a = 0.f, b = 0.f;
                if (Fn >= F || (f0 + v) % F < Fn) {
                    a = mag[ee];
                    if (HAS_PHI) {
                        float sn, cs;
                        sincosf(phase[ee], &sn, &cs);
                        b = a * sn, a = a * cs;
                    }
                }
                xre[ee] = a, xim[ee] = b;
            }
        }
    }
}

// sizes of a call: PSND_OK with grid == 0 when there is nothing to do
int gl_sizes(const char *who, int64_t N, int64_t K, int64_t F, unsigned &chunks, unsigned &M, unsigned &grid) {
    grid = 0;
    if (N < 0 || K < 0 || F < 0) PSND_FAIL(PSND_E_ARG, "%s: N=%lld K=%lld F=%lld", who, (long long)N, (long long)K, (long long)F);
    if (N == 0 || K == 0 || F == 0) return PSND_OK;
    if (K > 0x7fffffffll / F) PSND_FAIL(PSND_E_SHAPE, "%s: K=%lld F=%lld is 2^31 or more elements per item", who, (long long)K, (long long)F);
    const int64_t ch = psnd_gl_chunks(K, F);
    if (ch > 0x7fffffffll / N)
        PSND_FAIL(PSND_E_SHAPE, "%s: N=%lld K=%lld F=%lld is more than 2^31 - 1 workgroups", who, (long long)N, (long long)K, (long long)F);
    chunks = (unsigned)ch, M = (unsigned)(K * F), grid = (unsigned)(N * ch);
    return PSND_OK;
}

}  // namespace

extern "C" int64_t psnd_gl_chunk(void) { return CHUNK; }

extern "C" int64_t psnd_gl_chunks(int64_t K, int64_t F) {
    if (K <= 0 || F <= 0) return 0;
    if (K > INT64_MAX / F) return INT64_MAX;
    const int64_t M = K * F;
    return M / CHUNK + (M % CHUNK != 0);
}

extern "C" int psnd_griffinlim_start(const float *mag, const float *phase, int64_t N, int64_t K, int64_t F, const int64_t *frames,
                                     float *xre, float *xim, void *stream) {
    unsigned chunks, M, grid;
    const int rc = gl_sizes("griffinlim_start", N, K, F, chunks, M, grid);
    if (rc != PSND_OK || grid == 0) return rc;
    if (!mag || !xre || !xim) PSND_FAIL(PSND_E_ARG, "griffinlim_start: null pointer");
    const long long *fr = reinterpret_cast<const long long *>(frames);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (phase)
        hipLaunchKernelGGL(gl_start_kernel<true>, dim3(grid), dim3(THREADS), 0, st, mag, phase, chunks, M, (unsigned)F, fr, xre, xim);
    else
        hipLaunchKernelGGL(gl_start_kernel<false>, dim3(grid), dim3(THREADS), 0, st, mag, phase, chunks, M, (unsigned)F, fr, xre, xim);
    PSND_CHECK_LAUNCH("griffinlim_start");
    return PSND_OK;
}

extern "C" int psnd_griffinlim_step(const float *mag, const float *cre, const float *cim, const float *pre, const float *pim, int64_t N,
                                    int64_t K, int64_t F, const int64_t *frames, float alpha, float eps, float *xre, float *xim,
                                    float *partial, void *stream) {
    unsigned chunks, M, grid;
    const int rc = gl_sizes("griffinlim_step", N, K, F, chunks, M, grid);
    if (rc != PSND_OK || grid == 0) return rc;
    if ((pre == nullptr) != (pim == nullptr)) PSND_FAIL(PSND_E_ARG, "griffinlim_step: pre and pim come together or not at all");
    if (!mag || !cre || !cim || !xre || !xim) PSND_FAIL(PSND_E_ARG, "griffinlim_step: null pointer");
    const long long *fr = reinterpret_cast<const long long *>(frames);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(THREADS), 0, st, mag, cre, cim, pre, pim, chunks, M, (unsigned)F, fr, alpha, eps, xre, xim,
                           partial);
    };
    if (pre && partial) launch(gl_step_kernel<true, true>);
    else if (pre) launch(gl_step_kernel<true, false>);
    else if (partial) launch(gl_step_kernel<false, true>);
    else launch(gl_step_kernel<false, false>);
    PSND_CHECK_LAUNCH("griffinlim_step");
    return PSND_OK;
}
