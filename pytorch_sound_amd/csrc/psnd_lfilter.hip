// psnd_lfilter.hip - one recursive filter section of order <= 2 per row of an (N, T) fp32 tensor on gfx950, causal and mirrored in time:
// pytorch_sound/utils/sound.py preemphasis / inv_preemphasis (:66-71, scipy.signal.lfilter on the host) and the two-pole low-pass (:25-35).
//
//   y[t] = b0 x[t] + b1 x[t-1] + b2 x[t-2] - a1 y[t-1] - a2 y[t-2],   zero state before t = 0              (scipy's lfilter, zi = None)
//
// held in direct form II transposed:  y = b0 x + s1;  s1' = b1 x - a1 y + s2;  s2' = b2 x - a2 y.  With x = 0 the state moves by
// s' = M s, M = [[-a1, 1], [-a2, 0]], and the recurrence is LINEAR: a stretch of `len` samples entered with state s_in leaves with
//   s_out = M^len s_in + r,    r = the end state of the same stretch entered with the zero state.
// So stretches combine exactly (up to the rounding of fp64 products) - no warm-up, no truncation, any pole for which the powers stay
// finite, a pole on the unit circle included (an integrator's powers do not grow).  The tanh recurrence of psnd_sound.hip is parallel over
// time only by a contraction argument; this one needs none.
// The state and all products are fp64 (inputs and outputs fp32): the chain of a lane is latency bound either way (psnd_sound.hip), and the
// output is then the fp32 rounding of the fp64 trajectory that scipy computes.
//
// Parallel instance.  Geometry as psnd_sound.hip: a workgroup of 256 lanes owns a span of SPAN = 8192 samples of one row staged through the
// pitched LDS image (psnd_span_stage.h), a lane a chunk of CH = 32.
//   1. every lane walks its chunk from the zero state and keeps the end state r;
//   2. the 64 lanes of a wave combine by six shuffle steps (step k: lane l takes the state of lane l - 2^k through M^(32 2^k)), which leaves
//      in every lane the state at the end of its chunk for a wave entered with zero state;
//   3. the four waves combine through LDS with M^2048;
//   4. the spans of one row combine through memory and a LAUNCH BOUNDARY: lfilter_carry_kernel writes every span's zero-state end state
//      into carry[row][span][2]; lfilter_apply_kernel folds the carries of the spans before its own through M^8192 (at most a few hundred
//      2x2 products), repeats 1-3, gives every lane its true entry state and walks the chunk a second time, now storing y.
//   No workgroup waits on another inside a launch: no flags, no spinning, no atomics.  The second walk (32 dependent steps) is what that
//   costs.  A row of one span needs no carry and takes the second launch alone.
// The powers M^(32 2^k), k = 0..8, are formed on the host by repeated squaring in fp64 and travel by value with the five coefficients.
// reverse: the same filter with t+k for t-k.  Spans keep their place in memory; the order of chunks, lanes and spans is mirrored (thread j
// owns chunk 255 - j and walks it downwards, a span takes the carries of the spans behind it).  The zeros staged beyond T enter first
// there and leave the zero state as it is.
//
// Sequential instance: one workgroup per row, tiles of 8192 samples staged the same way (plain image), lane 0 walks.  For a pole so far
// outside the unit circle that M^8192 is not finite, and for coefficients that are not finite.  The host chooses (psnd.h).
#include "psnd_common.h"
#include "psnd_span_stage.h"

namespace {

constexpr int LANES = STAGE_LANES;
constexpr int CH = PSND_LFILTER_CHUNK;                  // samples per lane
constexpr int SPAN = PSND_LFILTER_SPAN;                 // samples per workgroup
constexpr int IMG = SPAN / 32 * 33;                     // words of the pitched LDS image
constexpr int LEVELS = 9;                               // M^(CH 2^k): k = 0..5 lanes of a wave, 6 waves of a workgroup, 8 spans of a row
static_assert(SPAN == LANES * CH && CH == 32 && LANES == 256 && (CH << 8) == SPAN, "geometry");

struct Mat2 {
    double m00, m01, m10, m11;
};
struct State {
    double s1, s2;
};
struct Section {
    double b0, b1, b2, a1, a2;
    Mat2 P[LEVELS];                                     // P[k] = M^(CH 2^k)
};

inline Mat2 mat_mul(const Mat2 &a, const Mat2 &b) {
    return {a.m00 * b.m00 + a.m01 * b.m10, a.m00 * b.m01 + a.m01 * b.m11, a.m10 * b.m00 + a.m11 * b.m10, a.m10 * b.m01 + a.m11 * b.m11};
}
// P s + r
__device__ __forceinline__ State carry_on(const Mat2 &P, const State &s, const State &r) {
    return {fma(P.m00, s.s1, fma(P.m01, s.s2, r.s1)), fma(P.m10, s.s1, fma(P.m11, s.s2, r.s2))};
}
__device__ __forceinline__ double step(const Section &c, State &s, double x) {
    const double y = fma(c.b0, x, s.s1);
    s.s1 = fma(-c.a1, y, fma(c.b1, x, s.s2));
    s.s2 = fma(-c.a2, y, c.b2 * x);
    return y;
}

// the chunk at words [p, p + CH) of the image, walked in the direction of the filter from state s; STORE: y replaces x in place
template <bool REV, bool STORE>
__device__ __forceinline__ State walk(const Section &c, float *s, int p, State st) {
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const int q = p + (REV ? CH - 1 - k : k);
        const double y = step(c, st, (double)s[q]);
        if (STORE) s[q] = (float)y;
    }
    return st;
}

// in: the zero-state end state of this thread's chunk.  out: the end state of its chunk for a WAVE entered with the zero state.  A lane
// only ever takes from lanes before it, by selection: what a later chunk holds (a NaN, say) never reaches an earlier one.
__device__ __forceinline__ State wave_scan(const Section &c, State r) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const State u = {__shfl_up(r.s1, 1u << k, 64), __shfl_up(r.s2, 1u << k, 64)};
        const State v = carry_on(c.P[k], u, r);
        if (lane >= (1 << k)) r = v;
    }
    return r;
}

// thread j owns chunk j of the span in filter order: the memory chunk j, or 255 - j mirrored
template <bool REV>
__device__ __forceinline__ int chunk_of_thread() {
    return REV ? LANES - 1 - (int)threadIdx.x : (int)threadIdx.x;
}

// stages the span and runs steps 1 and 2; tot[w] = end state of wave w entered with the zero state.  Returns this thread's scanned state.
template <bool REV>
__device__ __forceinline__ State span_scan(const Section &c, float *s, State *tot, const float *xr, long long T, long long b0, int cover) {
    stage_in<true>(s, xr, T, b0, cover);
    __syncthreads();
    const int ch = chunk_of_thread<REV>();
    State r = {0.0, 0.0};
    if (ch * CH < cover) r = walk<REV, false>(c, s, pitched(ch * CH), r);      // chunks beyond `cover` are not staged: zero input, zero state
    r = wave_scan(c, r);
    if ((threadIdx.x & 63) == 63) tot[threadIdx.x >> 6] = r;
    __syncthreads();
    return r;
}

// ---- launch 1: carry[row][span] = end state of the span entered with the zero state -------------------------------------------------------
template <bool REV>
__global__ __launch_bounds__(LANES) void lfilter_carry_kernel(const float *x, long long T, int spans, Section c, double *carry) {
    __shared__ __attribute__((aligned(16))) float s[IMG];
    __shared__ State tot[LANES / 64];
    const long long row = blockIdx.x / spans;
    const int span = (int)(blockIdx.x % spans);
    const long long b0 = (long long)span * SPAN;
    const int cover = (int)min((long long)SPAN, (T - b0 + 31) & ~31ll);
    span_scan<REV>(c, s, tot, x + (size_t)row * T, T, b0, cover);
    if (threadIdx.x == 0) {
        State e = tot[0];
        for (int w = 1; w < LANES / 64; ++w) e = carry_on(c.P[6], e, tot[w]);
        double *o = carry + ((size_t)row * spans + span) * 2;
        o[0] = e.s1, o[1] = e.s2;
    }
}

// ---- launch 2: the entry state of every chunk, the second walk, y -------------------------------------------------------------------------
template <bool REV>
__global__ __launch_bounds__(LANES) void lfilter_apply_kernel(const float *x, long long T, int spans, Section c, const double *carry, float *y) {
    __shared__ __attribute__((aligned(16))) float s[IMG];
    __shared__ State tot[LANES / 64];
    const long long row = blockIdx.x / spans;
    const int span = (int)(blockIdx.x % spans);
    const long long b0 = (long long)span * SPAN;
    const int cover = (int)min((long long)SPAN, (T - b0 + 31) & ~31ll);
    // the state this span is entered with: the spans before it in filter order, each a full span (only the last one in memory can be short,
    // and mirrored that one comes first)
    State in = {0.0, 0.0};
    const double *cr = carry + (size_t)row * spans * 2;
    if (REV) {
        for (int j = spans - 1; j > span; --j) in = carry_on(c.P[8], in, State{cr[2 * j], cr[2 * j + 1]});
    } else {
        for (int j = 0; j < span; ++j) in = carry_on(c.P[8], in, State{cr[2 * j], cr[2 * j + 1]});
    }
    const State r = span_scan<REV>(c, s, tot, x + (size_t)row * T, T, b0, cover);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int w = 0; w < wave; ++w) in = carry_on(c.P[6], in, tot[w]);           // entry state of this wave
    // entry state of this lane: the wave's entry state through M^(32 lane), the product of the levels at the set bits of `lane`, plus the
    // scanned state of the lane before it
    State ex = {__shfl_up(r.s1, 1u, 64), __shfl_up(r.s2, 1u, 64)};
    if (lane == 0) ex = State{0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const State v = carry_on(c.P[k], in, State{0.0, 0.0});
        if ((lane >> k) & 1) in = v;
    }
    in.s1 += ex.s1, in.s2 += ex.s2;
    const int ch = chunk_of_thread<REV>();
    if (ch * CH < cover) walk<REV, true>(c, s, pitched(ch * CH), in);
    __syncthreads();
    stage_out<true>(s, 0, y + (size_t)row * T, T, b0, cover);
}

// ---- sequential instance ------------------------------------------------------------------------------------------------------------------
template <bool REV>
__global__ __launch_bounds__(LANES) void lfilter_seq_kernel(const float *x, long long T, Section c, float *y) {
    __shared__ __attribute__((aligned(16))) float s[SPAN];
    const float *xr = x + (size_t)blockIdx.x * T;
    float *yr = y + (size_t)blockIdx.x * T;
    State st = {0.0, 0.0};
    for (long long done = 0; done < T; done += SPAN) {
        // forward: tiles from the start; mirrored: tiles from the end, with `t1` as the row's end so that nothing of the later tile is staged
        const long long t0 = REV ? max(0ll, T - done - SPAN) : done;
        const long long t1 = REV ? T - done : min(T, done + SPAN);
        const int n = (int)(t1 - t0), n4 = (n + 3) & ~3;
        stage_in<false>(s, xr, t1, t0, n4);
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; ++i) {
                const int q = REV ? n - 1 - i : i;
                s[q] = (float)step(c, st, (double)s[q]);
            }
        __syncthreads();
        stage_out<false>(s, 0, yr, t1, t0, n4);
        __syncthreads();
    }
}

}  // namespace

extern "C" int64_t psnd_lfilter_spans(int64_t T) { return T > 0 ? (T + SPAN - 1) / SPAN : 0; }

extern "C" int psnd_lfilter(const float *x, int64_t N, int64_t T, double b0, double b1, double b2, double a1, double a2, int reverse,
                            int instance, double *carry, float *y, void *stream) {
    if (N < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "lfilter: N=%lld T=%lld", (long long)N, (long long)T);
    if (instance != PSND_LFILTER_PARALLEL && instance != PSND_LFILTER_SEQ)
        PSND_FAIL(PSND_E_ARG, "lfilter: instance=%d (PSND_LFILTER_PARALLEL or PSND_LFILTER_SEQ)", instance);
    if (reverse != 0 && reverse != 1) PSND_FAIL(PSND_E_ARG, "lfilter: reverse=%d", reverse);
    if (N == 0 || T == 0) return PSND_OK;
    if (!x || !y) PSND_FAIL(PSND_E_ARG, "lfilter: null pointer");
    if (x == y) PSND_FAIL(PSND_E_ARG, "lfilter: x and y must be different buffers");
    if (instance == PSND_LFILTER_PARALLEL && !carry) PSND_FAIL(PSND_E_ARG, "lfilter: the parallel instance needs the carry scratch");
    const long long spans = psnd_lfilter_spans(T);
    if (N > 0x7fffffff || spans > 0x7fffffff || N * spans > 0x7fffffff)
        PSND_FAIL(PSND_E_SHAPE, "lfilter: N=%lld T=%lld is more than 2^31 - 1 workgroups", (long long)N, (long long)T);
    hipStream_t st = static_cast<hipStream_t>(stream);
    Section c = {b0, b1, b2, a1, a2, {}};
    if (instance == PSND_LFILTER_SEQ) {
        if (reverse)
            hipLaunchKernelGGL(lfilter_seq_kernel<true>, dim3((unsigned)N), dim3(LANES), 0, st, x, (long long)T, c, y);
        else
            hipLaunchKernelGGL(lfilter_seq_kernel<false>, dim3((unsigned)N), dim3(LANES), 0, st, x, (long long)T, c, y);
        PSND_CHECK_LAUNCH("lfilter (sequential instance)");
        return PSND_OK;
    }
    Mat2 p = {-a1, 1.0, -a2, 0.0};
    for (int i = 1; i < CH; i <<= 1) p = mat_mul(p, p);                  // M^32
    c.P[0] = p;
    for (int k = 1; k < LEVELS; ++k) c.P[k] = mat_mul(c.P[k - 1], c.P[k - 1]);
    const dim3 grid((unsigned)(N * spans));
    if (spans > 1) {
        if (reverse)
            hipLaunchKernelGGL(lfilter_carry_kernel<true>, grid, dim3(LANES), 0, st, x, (long long)T, (int)spans, c, carry);
        else
            hipLaunchKernelGGL(lfilter_carry_kernel<false>, grid, dim3(LANES), 0, st, x, (long long)T, (int)spans, c, carry);
        PSND_CHECK_LAUNCH("lfilter (span carries)");
    }
    if (reverse)
        hipLaunchKernelGGL(lfilter_apply_kernel<true>, grid, dim3(LANES), 0, st, x, (long long)T, (int)spans, c, (const double *)carry, y);
    else
        hipLaunchKernelGGL(lfilter_apply_kernel<false>, grid, dim3(LANES), 0, st, x, (long long)T, (int)spans, c, (const double *)carry, y);
    PSND_CHECK_LAUNCH("lfilter");
    return PSND_OK;
}
