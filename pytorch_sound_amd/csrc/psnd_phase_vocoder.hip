// psnd_phase_vocoder.hip - time-scale modification of an (N, K, F) fp32 complex spectrogram on gfx950 by the definition of include/psnd.h:
// output frame j of a row reads the input frames i = floor(j rate) and i + 1, interpolates their magnitudes and advances its phase by
// arg X[i + 1] - arg X[i] of the frame before it.  What stands between STFT.transform_complex and STFT.inverse_complex in
// utils.sound.time_stretch / pitch_shift.
//
// One launch, no scratch, no atomics.  A workgroup of WAVES = 4 waves takes 4 consecutive rows, one wave per row; nothing is exchanged
// between the waves.  A wave walks its row in passes of PASS = 64 x V consecutive output frames, lane l the V = 4 frames
// j0 + 4 l .. j0 + 4 l + 3, so that its results leave in one 16-byte store per part.  i_j is monotone in j: the lanes of a pass read a
// span of about PASS rate consecutive elements, every cache line of it once from memory.
//   The phase is a prefix sum over the whole row, and a row may have thousands of frames: summed as fp32 angles it drifts (2e-3 at 2800
//   frames).  Here every angle becomes a 64-bit fixed-point fraction of a turn (2^64 = one turn) right behind atan2f; a step is the
//   difference of two such numbers, the sum of steps is integer addition - exact, in any order, and the wrap-around of the integer IS the
//   reduction modulo a turn.  Per pass: V - 1 additions inside the lane, a shuffle scan of the lane totals, a carried total.
//   "NaN from the first frame that reads a non-finite element on" is a prefix OR along the same road: a ballot per pass and a carried flag.
// Frames at or behind the row's count (t_j >= F_n) read nothing and store (0, 0); a pass that lies wholly behind it skips the arithmetic.
#include "psnd_common.h"

namespace {

constexpr int WAVES = 4;
constexpr int V = 4;
constexpr int PASS = 64 * V;

typedef unsigned long long u64;

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// arg (re + i im) as a fraction of a turn, 2^64 = one turn; arg 0 = 0 whatever the signs of the zeros; 0 for an element that is not finite
// (its row is NaN from there on by the flag, the number is never shown)
__device__ __forceinline__ u64 arg_turns(float re, float im, bool finite) {
    if (!finite || (re == 0.f && im == 0.f)) return 0;
    const double turns = (double)atan2f(im, re) * 0.15915494309189535;          // [-1/2, 1/2] and a rounding
    return (u64)(long long)rint(turns * 9223372036854775808.0) << 1;            // |turns 2^63| <= 2^62 + : inside int64
}

__global__ __launch_bounds__(64 * WAVES) void pv_kernel(const float *__restrict__ re, const float *__restrict__ im, long long rows,
                                                        long long K, long long F, const long long *__restrict__ frames, double rate,
                                                        float *__restrict__ yre, float *__restrict__ yim, long long J) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    long long Fn = F;
    if (frames) {
        const long long v = frames[row / K];
        Fn = v < 0 ? 0 : (v > F ? F : v);
    }
    const float *xr = re + (size_t)row * F, *xi = im + (size_t)row * F;
    float *outr = yre + (size_t)row * J, *outi = yim + (size_t)row * J;
    const double Fd = (double)Fn;
    u64 carry = 0;                                      // phi of the first frame of the pass, before the steps inside it
    bool carry_bad = false;                             // a frame of an earlier pass read a non-finite element
    for (long long j0 = 0; j0 < J; j0 += PASS) {
        const long long jb = j0 + (long long)lane * V;
        const bool whole = jb + V <= J;                 // this lane's four slots all exist
        // validity is monotone in j: the pass is dead when its first frame is
        if (!(__dmul_rn((double)j0, rate) < Fd)) {
            if (whole) {
                *reinterpret_cast<f32x4_u *>(outr + jb) = f32x4_u{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4_u *>(outi + jb) = f32x4_u{0.f, 0.f, 0.f, 0.f};
            } else {
                for (int v = 0; v < V; ++v)
                    if (jb + v < J) outr[jb + v] = 0.f, outi[jb + v] = 0.f;
            }
            continue;
        }
        float mag[V];
        u64 step[V];
        bool bad[V], valid[V];
        u64 first = 0;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const long long j = jb + v;
            const double t = __dmul_rn((double)j, rate);                       // ONE multiplication: never contracted with the subtraction
            valid[v] = j < J && t < Fd;
            mag[v] = 0.f, step[v] = 0, bad[v] = false;
            if (valid[v]) {
                const long long i = (long long)t;                               // 0 <= t < F_n: truncation is floor, i <= F_n - 1
                const float al = (float)(t - (double)i);
                const bool has = i + 1 < Fn;
                const float ar = xr[i], ai = xi[i];
                const float br = has ? xr[i + 1] : 0.f, bi = has ? xi[i + 1] : 0.f;
                const bool fa = finite_bits(ar) && finite_bits(ai), fb = finite_bits(br) && finite_bits(bi);
                mag[v] = (1.f - al) * hypotf(ar, ai) + al * hypotf(br, bi);
                const u64 pa = arg_turns(ar, ai, fa), pb = arg_turns(br, bi, fb);
                step[v] = pb - pa;
                bad[v] = !(fa && fb);
                if (j == 0) first = pa;
            }
        }
        if (j0 == 0) carry = __shfl(first, 0, 64);                              // phi_0 = arg X[0]
        // exclusive prefix of the steps: inside the lane, then across the lanes
        u64 ex[V];
        u64 tot = 0;
        bool any = false;
#pragma unroll
        for (int v = 0; v < V; ++v) {
            ex[v] = tot;
            tot += step[v];
            any |= bad[v];
            bad[v] = any;                                                       // inclusive: a frame is lost through its own reads too
        }
        u64 inc = tot;
#pragma unroll
        for (int k = 1; k < 64; k <<= 1) {
            const u64 up = __shfl_up(inc, k, 64);
            if (lane >= k) inc += up;
        }
        const u64 base = carry + (inc - tot);
        const unsigned long long lost = __ballot(any);
        const bool before = carry_bad || (lost & ((1ull << lane) - 1ull)) != 0;
        carry += __shfl(inc, 63, 64);
        carry_bad = carry_bad || lost != 0;
        float o_r[V], o_i[V];
        const float nan = __int_as_float(0x7fc00000);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const long long ph = (long long)(base + ex[v]);                     // [-2^63, 2^63) = [-1/2, 1/2) of a turn
            const float ang = (float)((double)ph * 3.4061215800865545e-19);     // 2 pi / 2^64
            float sn, cs;
            sincosf(ang, &sn, &cs);
            const bool nn = before || bad[v];
            o_r[v] = !valid[v] ? 0.f : (nn ? nan : mag[v] * cs);
            o_i[v] = !valid[v] ? 0.f : (nn ? nan : mag[v] * sn);
        }
        if (whole) {
            *reinterpret_cast<f32x4_u *>(outr + jb) = f32x4_u{o_r[0], o_r[1], o_r[2], o_r[3]};
            *reinterpret_cast<f32x4_u *>(outi + jb) = f32x4_u{o_i[0], o_i[1], o_i[2], o_i[3]};
        } else {
#pragma unroll
            for (int v = 0; v < V; ++v)
                if (jb + v < J) outr[jb + v] = o_r[v], outi[jb + v] = o_i[v];
        }
    }
}

}  // namespace

extern "C" int64_t psnd_pv_pass(void) { return PASS; }

extern "C" int64_t psnd_pv_frames(int64_t F, double rate) {
    if (F <= 0 || !(rate > 0.0) || !(rate < __builtin_inf())) return 0;
    const double q = __builtin_ceil((double)F / rate);
    if (!(q < 9007199254740992.0)) return INT64_MAX;
    int64_t j = (int64_t)q;                             // the count is the smallest j with (double) j * rate >= F: j * rate is monotone in j
    while (j > 0 && !((double)(j - 1) * rate < (double)F)) --j;
    while ((double)j * rate < (double)F) ++j;
    return j;
}

extern "C" int psnd_phase_vocoder(const float *re, const float *im, int64_t N, int64_t K, int64_t F, const int64_t *frames, double rate,
                                  float *yre, float *yim, int64_t J, void *stream) {
    if (!(rate > 0.0) || !(rate < __builtin_inf())) PSND_FAIL(PSND_E_ARG, "phase_vocoder: rate=%g (positive and finite)", rate);
    if (N < 0 || K < 0 || F < 0) PSND_FAIL(PSND_E_ARG, "phase_vocoder: N=%lld K=%lld F=%lld", (long long)N, (long long)K, (long long)F);
    if (J < 0 || J >= (1ll << 31)) PSND_FAIL(PSND_E_ARG, "phase_vocoder: J=%lld output frames (0 <= J < 2^31)", (long long)J);
    if (J < psnd_pv_frames(F, rate))
        PSND_FAIL(PSND_E_ARG, "phase_vocoder: J=%lld, a row of F=%lld frames at rate=%g has psnd_pv_frames = %lld", (long long)J, (long long)F,
                  rate, (long long)psnd_pv_frames(F, rate));
    if (N == 0 || K == 0 || J == 0) return PSND_OK;
    if (((!re || !im) && F > 0) || !yre || !yim) PSND_FAIL(PSND_E_ARG, "phase_vocoder: null pointer");
    if (K > INT64_MAX / N || (N * K + WAVES - 1) / WAVES > 0x7fffffffll)
        PSND_FAIL(PSND_E_SHAPE, "phase_vocoder: N=%lld K=%lld is more than 2^31 - 1 workgroups", (long long)N, (long long)K);
    const long long rows = (long long)(N * K);
    hipLaunchKernelGGL(pv_kernel, dim3((unsigned)((rows + WAVES - 1) / WAVES)), dim3(64 * WAVES), 0, static_cast<hipStream_t>(stream), re, im,
                       rows, (long long)K, (long long)F, reinterpret_cast<const long long *>(frames), rate, yre, yim, (long long)J);
    PSND_CHECK_LAUNCH("phase_vocoder");
    return PSND_OK;
}
