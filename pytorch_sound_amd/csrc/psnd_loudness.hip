// psnd_loudness.hip - ITU-R BS.1770-4 / EBU R128 integrated loudness, plain levels and per-programme gain on (N C, T) fp32 rows on gfx950.
// The definition is in include/psnd.h.  The reference levels its files on the host (scripts/preprocess.py:32-41, ffmpeg-normalize).
//
// psnd_loudness.  The K-weighting is two sections of order 2 in series.  Held in direct form II transposed as psnd_lfilter.hip holds one, the
// cascade has the state (s1, s2, u1, u2) and with x = 0 it moves by v' = M v,
//        M = | A  0 |     A = [[-a1, 1], [-a2, 0]] of the shelf, D the same of the high-pass (g, h its b, a),
//            | C  D |     C = [[g1 - h1 g0, 0], [g2 - h2 g0, 0]]           (the shelf's output with x = 0 is s1),
// so a stretch of `len` samples entered with v_in leaves with M^len v_in + r, r = its end state entered with zero: the exact scan of
// psnd_lfilter.hip over both sections at once, in fp64, with the same geometry (a workgroup of 256 lanes owns a span of 8192 samples staged
// through the pitched LDS image, a lane a chunk of 32; lanes combine by shuffles, waves through LDS, spans through carry[row][span][4] and a
// launch boundary).  Powers of M keep the block-triangular form: 12 doubles each, formed on the host by squaring.
//   1  carry_kernel   (rows with more than one span) every span's zero-state end state.
//   2  energy_kernel  the entry state of every chunk, then the second walk: y is squared in registers and summed in fp64 into PIECES.  The
//                     piece ends are the multiples of H and, where R = B mod H > 0, those plus R: block j is then a whole number of
//                     consecutive pieces for any B >= H.  A lane's chunk holds the tail `a` of the piece of its first sample, pieces that
//                     lie wholly inside it (stored straight away), and the head `b` of the piece of its last sample.  v = a + b of the lane
//                     before is summed over the lanes of equal piece by a segmented scan (shuffles, then the four waves in ascending
//                     order through LDS); the lane that holds a piece's end, and the last lane, store part[row][span][piece - first piece
//                     of the span].  Every slot of a span is stored exactly once, in an order that never depends on timing.
//   3  final_kernel   one workgroup per programme: z[j] = sum over channels, pieces and the spans a piece crosses, all ascending; the two
//                     gated means as per-lane sums over j = lane, lane + 256, ... folded by a fixed tree; lufs, blocks, gain.  z is formed
//                     again in the second pass (the same sums, the same bits) instead of being kept: J_r is unbounded.
// The filtered signal never reaches memory; no atomics, no workgroup waits on another inside a launch.  A non-finite sample enters the filter
// as 0 and raises its span's flag: the programme reads NaN, no other programme sees it.
//
// psnd_row_level: one workgroup of 1024 lanes per programme, fp64 sum of squares and max |x| per lane over t = 4 lane, 4 lane + 4096, ...,
// folded by a fixed tree.  psnd_gain_rows: y = x gain[row / C] before the programme's length, y = x behind it.
#include "psnd_common.h"
#include "psnd_span_stage.h"
#include <math.h>

namespace {

constexpr int LANES = STAGE_LANES;
constexpr int WAVES = LANES / 64;
constexpr int CH = 32;                                  // samples per lane
constexpr int SPAN = LANES * CH;                        // samples per workgroup
constexpr int IMG = SPAN / 32 * 33;                     // words of the pitched LDS image
constexpr int LEVELS = 9;                               // M^(CH 2^k): k = 0..5 lanes of a wave, 6 waves of a workgroup, 8 spans of a row
constexpr int MAX_C = 32;                               // channel weights travel by value
constexpr int LV_LANES = 1024;
constexpr int GAIN_PER = 4 * LANES;                     // samples per workgroup of gain_kernel
static_assert(SPAN == 8192 && (CH << 8) == SPAN, "geometry");

struct Sec {
    double b0, b1, b2, a1, a2;
};
struct Mat4 {                                           // [[A, 0], [C, D]], 2 x 2 blocks row-major
    double a[4], c[4], d[4];
};
struct State {
    double s1, s2, u1, u2;
};
struct Filt {
    Sec f, g;                                           // shelf, high-pass
    Mat4 P[LEVELS];                                     // P[k] = M^(CH 2^k)
};
struct Weights {
    double g[MAX_C];
};

inline void mul2(const double *x, const double *y, double *o) {
    o[0] = x[0] * y[0] + x[1] * y[2], o[1] = x[0] * y[1] + x[1] * y[3];
    o[2] = x[2] * y[0] + x[3] * y[2], o[3] = x[2] * y[1] + x[3] * y[3];
}
inline Mat4 mat_mul(const Mat4 &x, const Mat4 &y) {       // x y
    Mat4 o;
    double t0[4], t1[4];
    mul2(x.a, y.a, o.a);
    mul2(x.d, y.d, o.d);
    mul2(x.c, y.a, t0);
    mul2(x.d, y.c, t1);
    for (int i = 0; i < 4; ++i) o.c[i] = t0[i] + t1[i];
    return o;
}

// P v + r
__device__ __forceinline__ State carry_on(const Mat4 &P, const State &v, const State &r) {
    State o;
    o.s1 = fma(P.a[0], v.s1, fma(P.a[1], v.s2, r.s1));
    o.s2 = fma(P.a[2], v.s1, fma(P.a[3], v.s2, r.s2));
    o.u1 = fma(P.c[0], v.s1, fma(P.c[1], v.s2, fma(P.d[0], v.u1, fma(P.d[1], v.u2, r.u1))));
    o.u2 = fma(P.c[2], v.s1, fma(P.c[3], v.s2, fma(P.d[2], v.u1, fma(P.d[3], v.u2, r.u2))));
    return o;
}
__device__ __forceinline__ double step(const Filt &c, State &v, double x) {
    const double y = fma(c.f.b0, x, v.s1);
    v.s1 = fma(-c.f.a1, y, fma(c.f.b1, x, v.s2));
    v.s2 = fma(-c.f.a2, y, c.f.b2 * x);
    const double w = fma(c.g.b0, y, v.u1);
    v.u1 = fma(-c.g.a1, w, fma(c.g.b1, y, v.u2));
    v.u2 = fma(-c.g.a2, w, c.g.b2 * y);
    return w;
}
__device__ __forceinline__ bool non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ long long prog_len(const long long *lengths, long long prog, long long T) {
    if (!lengths) return T;
    const long long v = lengths[prog];
    return v < 0 ? 0 : (v > T ? T : v);
}

// the first walk of a lane's chunk from the zero state; bad: a non-finite sample was met (it enters as 0)
__device__ __forceinline__ State walk_state(const Filt &c, const float *s, int p, bool &bad) {
    State v = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const float x = s[p + k];
        const bool nf = non_finite(x);
        bad |= nf;
        step(c, v, nf ? 0.0 : (double)x);
    }
    return v;
}

// in: the zero-state end state of this lane's chunk.  out: the end state of its chunk for a WAVE entered with the zero state
__device__ __forceinline__ State wave_scan(const Filt &c, State r) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const State u = {__shfl_up(r.s1, 1u << k, 64), __shfl_up(r.s2, 1u << k, 64), __shfl_up(r.u1, 1u << k, 64), __shfl_up(r.u2, 1u << k, 64)};
        const State v = carry_on(c.P[k], u, r);
        if (lane >= (1 << k)) r = v;
    }
    return r;
}

// stages the span (zeros behind `len`), walks, scans; tot[w] = end state of wave w entered with the zero state
__device__ __forceinline__ State span_scan(const Filt &c, float *s, State *tot, const float *xr, long long len, long long b0, bool &bad) {
    stage_in<true>(s, xr, len, b0, SPAN);
    __syncthreads();
    State r = walk_state(c, s, pitched((int)threadIdx.x * CH), bad);
    r = wave_scan(c, r);
    if ((threadIdx.x & 63) == 63) tot[threadIdx.x >> 6] = r;
    __syncthreads();
    return r;
}

// ---- launch 1 -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void loudness_carry_kernel(const float *x, long long T, const long long *lengths, int C, int spans, Filt c,
                                                               double *carry) {
    __shared__ __attribute__((aligned(16))) float s[IMG];
    __shared__ State tot[WAVES];
    const long long row = blockIdx.x / spans;
    const int span = (int)(blockIdx.x % spans);
    const long long b0 = (long long)span * SPAN;
    const long long len = prog_len(lengths, row / C, T);
    double *o = carry + ((size_t)row * spans + span) * 4;
    if (b0 >= len) {                                    // the whole workgroup: nothing behind the length is read
        if (threadIdx.x < 4) o[threadIdx.x] = 0.0;
        return;
    }
    bool bad = false;
    span_scan(c, s, tot, x + (size_t)row * T, len, b0, bad);
    if (threadIdx.x == 0) {
        State e = tot[0];
        for (int w = 1; w < WAVES; ++w) e = carry_on(c.P[6], e, tot[w]);
        o[0] = e.s1, o[1] = e.s2, o[2] = e.u1, o[3] = e.u2;
    }
}

// the index of the piece that holds sample t: hops of H, each cut at R where R > 0
__host__ __device__ inline long long piece_of(long long t, long long H, long long R) {
    const long long q = t / H;
    return R ? 2 * q + (t - q * H >= R) : q;
}
__host__ __device__ inline long long piece_slots(long long H, long long R) { return (R ? 2 : 1) * (SPAN / H + 2); }

// ---- launch 2 -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void loudness_energy_kernel(const float *x, long long T, const long long *lengths, int C, int spans, Filt c,
                                                                long long H, long long R, const double *carry, double *part, int *flag) {
    __shared__ __attribute__((aligned(16))) float s[IMG];
    __shared__ State tot[WAVES];
    __shared__ double lb[LANES];
    __shared__ double wt[WAVES];
    __shared__ int wk[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row = blockIdx.x / spans;
    const int span = (int)(blockIdx.x % spans);
    const long long b0 = (long long)span * SPAN;
    const long long len = prog_len(lengths, row / C, T);
    const long long slots = piece_slots(H, R);
    double *pr = part + ((size_t)row * spans + span) * slots;
    if (b0 >= len) {                                    // the whole workgroup
        for (long long j = tid; j < slots; j += LANES) pr[j] = 0.0;
        if (tid == 0) flag[(size_t)row * spans + span] = 0;
        return;
    }
    State in = {0.0, 0.0, 0.0, 0.0};                    // the state this span is entered with
    const double *cr = carry + (size_t)row * spans * 4;
    for (int j = 0; j < span; ++j) in = carry_on(c.P[8], in, State{cr[4 * j], cr[4 * j + 1], cr[4 * j + 2], cr[4 * j + 3]});
    bool bad = false;
    const State r = span_scan(c, s, tot, x + (size_t)row * T, len, b0, bad);
    for (int w = 0; w < wave; ++w) in = carry_on(c.P[6], in, tot[w]);           // entry state of this wave
    State ex = {__shfl_up(r.s1, 1u, 64), __shfl_up(r.s2, 1u, 64), __shfl_up(r.u1, 1u, 64), __shfl_up(r.u2, 1u, 64)};
    if (lane == 0) ex = State{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) {                       // through M^(32 lane)
        const State v = carry_on(c.P[k], in, State{0.0, 0.0, 0.0, 0.0});
        if ((lane >> k) & 1) in = v;
    }
    in.s1 += ex.s1, in.s2 += ex.s2, in.u1 += ex.u1, in.u2 += ex.u2;

    // the second walk: squares into pieces
    const long long t0 = b0 + (long long)tid * CH;
    const long long p_span = piece_of(b0, H, R);
    const int key = (int)(piece_of(t0, H, R) - p_span);  // the slot of the piece of this lane's first sample
    long long m = t0 % H;
    int slot = key;
    bool had_end = false;
    double acc = 0.0, a = 0.0;
    const int p = pitched(tid * CH);
#pragma unroll 8
    for (int k = 0; k < CH; ++k) {
        const float xv = s[p + k];
        const double y = step(c, in, non_finite(xv) ? 0.0 : (double)xv);
        acc = fma(y, y, acc);
        if (++m == H) m = 0;
        if (m == 0 || m == R) {                         // sample t0 + k closes its piece
            if (!had_end)
                a = acc, had_end = true;
            else
                pr[slot] = acc;                         // a piece wholly inside this chunk
            acc = 0.0;
            ++slot;
        }
    }
    const double b = had_end ? acc : 0.0;               // the open piece behind the last end (empty: 0)
    if (!had_end) a = acc;
    lb[tid] = b;
    const int any_bad = __syncthreads_or(bad);
    double v = a + (tid > 0 ? lb[tid - 1] : 0.0);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                  // keys ascend with the lane: equal keys are neighbours
        const double vo = __shfl_up(v, d, 64);
        const int ko = __shfl_up(key, d, 64);
        if (lane >= d && ko == key) v += vo;
    }
    if (lane == 63) wt[wave] = v, wk[wave] = key;
    __syncthreads();
    double before = 0.0;
    for (int w = 0; w < wave; ++w)
        if (wk[w] == key) before += wt[w];
    v = before + v;
    if (had_end || tid == LANES - 1) pr[key] = v;
    // the last lane's open piece, unless the span ends on a piece end
    if (tid == LANES - 1 && had_end && (long long)slot == piece_of(b0 + SPAN - 1, H, R) - p_span) pr[slot] = b;
    if (tid == 0) flag[(size_t)row * spans + span] = any_bad;
}

// ---- launch 3 -----------------------------------------------------------------------------------------------------------------------------
struct Geo {
    long long T, B, H, R, Jmax;
    int C, spans;
};

// the energy of piece p of one row: the spans it crosses, ascending
__device__ __forceinline__ double piece_energy(const double *part_row, const Geo &g, long long slots, long long p) {
    long long lo, hi;                                   // [lo, hi)
    if (g.R) {
        const long long q = p >> 1;
        lo = q * g.H + ((p & 1) ? g.R : 0);
        hi = (p & 1) ? (q + 1) * g.H : q * g.H + g.R;
    } else {
        lo = p * g.H, hi = lo + g.H;
    }
    double e = 0.0;
    for (long long sp = lo / SPAN; sp <= (hi - 1) / SPAN && sp < g.spans; ++sp)
        e += part_row[(size_t)sp * slots + (p - piece_of(sp * SPAN, g.H, g.R))];
    return e;
}

// z[j] of a programme whose first row's pieces are at part_prog
__device__ __forceinline__ double block_energy(const double *part_prog, const Geo &g, const Weights &G, long long slots, long long j) {
    const long long m = g.B / g.H;
    const long long p0 = g.R ? 2 * j : j, p1 = g.R ? 2 * (j + m) : j + m - 1;   // inclusive
    double z = 0.0;
    for (int ch = 0; ch < g.C; ++ch) {
        const double *pr = part_prog + (size_t)ch * g.spans * slots;
        double e = 0.0;
        for (long long p = p0; p <= p1; ++p) e += piece_energy(pr, g, slots, p);
        z = fma(G.g[ch], e, z);
    }
    return z / (double)g.B;
}

// the sum of v and of n over the workgroup by a fixed tree; every lane gets both
__device__ __forceinline__ void fold(double *sv, long long *sn, double &v, long long &n) {
    const int tid = threadIdx.x;
    sv[tid] = v, sn[tid] = n;
    __syncthreads();
    for (int d = LANES / 2; d > 0; d >>= 1) {
        if (tid < d) sv[tid] += sv[tid + d], sn[tid] += sn[tid + d];
        __syncthreads();
    }
    v = sv[0], n = sn[0];
    __syncthreads();
}

__global__ __launch_bounds__(LANES) void loudness_final_kernel(const long long *lengths, Geo g, Weights G, double gate, double target, const double *part,
                                                               const int *flag, float *lufs, float *blocks, float *gain) {
    __shared__ double sv[LANES];
    __shared__ long long sn[LANES];
    const int tid = threadIdx.x;
    const long long prog = blockIdx.x;
    const long long len = prog_len(lengths, prog, g.T);
    const long long J = len < g.B ? 0 : (len - g.B) / g.H + 1;
    const long long slots = piece_slots(g.H, g.R);
    const double *pp = part + (size_t)prog * g.C * g.spans * slots;
    int bad = 0;
    for (long long i = tid; i < (long long)g.C * g.spans; i += LANES) bad |= flag[(size_t)prog * g.C * g.spans + i];
    bad = __syncthreads_or(bad);
    const float nanf_ = __uint_as_float(0x7fc00000u);
    double sum = 0.0;
    long long cnt = 0;
    for (long long j = tid; j < J; j += LANES) {
        const double z = block_energy(pp, g, G, slots, j);
        if (z > gate) sum += z, ++cnt;
        if (blocks) blocks[(size_t)prog * g.Jmax + j] = bad ? nanf_ : (float)z;
    }
    if (blocks)
        for (long long j = J + tid; j < g.Jmax; j += LANES) blocks[(size_t)prog * g.Jmax + j] = 0.f;
    fold(sv, sn, sum, cnt);
    double L = -INFINITY;
    if (cnt > 0) {                                      // uniform
        const double thr = 0.1 * (sum / (double)cnt);
        double sum2 = 0.0;
        long long cnt2 = 0;
        for (long long j = tid; j < J; j += LANES) {
            const double z = block_energy(pp, g, G, slots, j);
            if (z > gate && z > thr) sum2 += z, ++cnt2;
        }
        fold(sv, sn, sum2, cnt2);
        if (cnt2 > 0) L = -0.691 + 10.0 * log10(sum2 / (double)cnt2);
    }
    if (tid == 0) {
        const float Lf = bad ? nanf_ : (float)L;
        lufs[prog] = Lf;
        if (gain) gain[prog] = (bad || !(L > -INFINITY) || !(L < INFINITY)) ? 1.f : (float)pow(10.0, (target - (double)Lf) / 20.0);
    }
}

// ---- plain levels -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LV_LANES) void row_level_kernel(const float *x, long long T, const long long *lengths, int C, int of_peak,
                                                             double target, float *rms_db, float *peak_db, float *gain) {
    __shared__ double sv[LV_LANES];
    __shared__ float sm[LV_LANES];
    __shared__ int sb[LV_LANES];
    const int tid = threadIdx.x;
    const long long prog = blockIdx.x;
    const long long len = prog_len(lengths, prog, T);
    double sum = 0.0;
    float mx = 0.f;
    int bad = 0;
    for (int ch = 0; ch < C; ++ch) {
        const float *xr = x + ((size_t)prog * C + ch) * T;
        for (long long t = 4ll * tid; t < len; t += 4ll * LV_LANES) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (t + 3 < len) {
                v = *reinterpret_cast<const f32x4_u *>(xr + t);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (t + k < len) v[k] = xr[t + k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool nf = non_finite(v[k]);
                bad |= nf;
                const float f = nf ? 0.f : v[k];
                sum = fma((double)f, (double)f, sum);
                mx = fmaxf(mx, fabsf(f));
            }
        }
    }
    sv[tid] = sum, sm[tid] = mx, sb[tid] = bad;
    __syncthreads();
    for (int d = LV_LANES / 2; d > 0; d >>= 1) {
        if (tid < d) sv[tid] += sv[tid + d], sm[tid] = fmaxf(sm[tid], sm[tid + d]), sb[tid] |= sb[tid + d];
        __syncthreads();
    }
    if (tid == 0) {
        const double n = (double)len * (double)C;
        const float nanf_ = __uint_as_float(0x7fc00000u);
        const double r = n > 0.0 && sv[0] > 0.0 ? 10.0 * log10(sv[0] / n) : -INFINITY;
        const double pk = sm[0] > 0.f ? 20.0 * log10((double)sm[0]) : -INFINITY;
        const float rf = sb[0] ? nanf_ : (float)r, pf = sb[0] ? nanf_ : (float)pk;
        if (rms_db) rms_db[prog] = rf;
        if (peak_db) peak_db[prog] = pf;
        if (gain) {
            const float Lf = of_peak ? pf : rf;
            gain[prog] = (sb[0] || !(Lf > -INFINITY)) ? 1.f : (float)pow(10.0, (target - (double)Lf) / 20.0);
        }
    }
}

__global__ __launch_bounds__(LANES) void gain_rows_kernel(const float *x, long long T, const long long *lengths, int C, int chunks,
                                                          const float *gain, float *y) {
    const long long row = blockIdx.x / chunks;
    const long long t = (long long)(blockIdx.x % chunks) * GAIN_PER + 4ll * threadIdx.x;
    if (t >= T) return;
    const long long prog = row / C;
    const long long len = prog_len(lengths, prog, T);
    const float g = gain[prog];
    const float *xr = x + (size_t)row * T;
    float *yr = y + (size_t)row * T;
    if (t + 3 < T) {
        f32x4 v = *reinterpret_cast<const f32x4_u *>(xr + t);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (t + k < len) v[k] *= g;
        *reinterpret_cast<f32x4_u *>(yr + t) = v;
    } else {
        for (int k = 0; k < 4 && t + k < T; ++k) yr[t + k] = t + k < len ? xr[t + k] * g : xr[t + k];
    }
}

inline bool finite_all(const double *v, int n) {
    for (int i = 0; i < n; ++i)
        if (!isfinite(v[i])) return false;
    return true;
}
inline long long n_spans(long long T) { return T > 0 ? (T + SPAN - 1) / SPAN : 0; }
inline size_t pad16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

extern "C" int64_t psnd_loudness_span(void) { return SPAN; }
extern "C" int64_t psnd_loudness_max_channels(void) { return MAX_C; }

extern "C" int64_t psnd_loudness_blocks(int64_t T, int64_t B, int64_t H) {
    if (B < 1 || H < 1 || T < B) return 0;
    return (T - B) / H + 1;
}

extern "C" size_t psnd_loudness_scratch_bytes(int64_t N, int64_t C, int64_t T, int64_t B, int64_t H) {
    if (N <= 0 || C <= 0 || T <= 0 || B < 1 || H < 1 || H > B) return 0;
    const size_t rs = (size_t)N * (size_t)C * (size_t)n_spans(T);       // (row, span) pairs
    return pad16(rs * 4 * sizeof(double)) + pad16(rs * (size_t)piece_slots(H, B % H) * sizeof(double)) + pad16(rs * sizeof(int));
}

extern "C" int psnd_loudness(const float *x, int64_t N, int64_t C, int64_t T, const int64_t *lengths, double sb0, double sb1, double sb2,
                             double sa1, double sa2, double hb0, double hb1, double hb2, double ha1, double ha2, int64_t B, int64_t H,
                             const double *weights, double target, void *scratch, float *lufs, float *blocks, float *gain, void *stream) {
    if (B < 1 || H < 1 || H > B) PSND_FAIL(PSND_E_ARG, "loudness: B=%lld H=%lld (1 <= H <= B)", (long long)B, (long long)H);
    if (C < 1) PSND_FAIL(PSND_E_ARG, "loudness: C=%lld", (long long)C);
    if (N < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "loudness: N=%lld T=%lld", (long long)N, (long long)T);
    const double co[10] = {sb0, sb1, sb2, sa1, sa2, hb0, hb1, hb2, ha1, ha2};
    if (!finite_all(co, 10)) PSND_FAIL(PSND_E_ARG, "loudness: a filter coefficient is not finite");
    if (!isfinite(target)) PSND_FAIL(PSND_E_ARG, "loudness: target is not finite");
    if (C > MAX_C) PSND_FAIL(PSND_E_UNSUPPORTED, "loudness: C=%lld, at most %d channels per programme", (long long)C, MAX_C);
    if (!weights && C > 5) PSND_FAIL(PSND_E_ARG, "loudness: C=%lld needs explicit channel weights (the default covers 5)", (long long)C);
    Weights G = {};
    static const double dflt[5] = {1.0, 1.0, 1.0, 1.41, 1.41};
    for (int i = 0; i < (int)C; ++i) G.g[i] = weights ? weights[i] : dflt[i];
    if (!finite_all(G.g, (int)C)) PSND_FAIL(PSND_E_ARG, "loudness: a channel weight is not finite");
    if (N == 0 || T == 0) return PSND_OK;
    if (!x || !lufs || !scratch) PSND_FAIL(PSND_E_ARG, "loudness: null pointer");
    if ((uintptr_t)scratch % 16) PSND_FAIL(PSND_E_ARG, "loudness: scratch must be 16-byte aligned");
    const long long spans = n_spans(T);
    if (N > 0x7fffffff / C || N * C > 0x7fffffff / spans)
        PSND_FAIL(PSND_E_SHAPE, "loudness: N=%lld C=%lld T=%lld is more than 2^31 - 1 workgroups", (long long)N, (long long)C, (long long)T);
    Filt c = {{sb0, sb1, sb2, sa1, sa2}, {hb0, hb1, hb2, ha1, ha2}, {}};
    Mat4 p = {{-sa1, 1.0, -sa2, 0.0}, {hb1 - ha1 * hb0, 0.0, hb2 - ha2 * hb0, 0.0}, {-ha1, 1.0, -ha2, 0.0}};
    for (int i = 1; i < CH; i <<= 1) p = mat_mul(p, p);                 // M^32
    c.P[0] = p;
    for (int k = 1; k < LEVELS; ++k) c.P[k] = mat_mul(c.P[k - 1], c.P[k - 1]);
    for (int k = 0; k < LEVELS; ++k)
        if (!finite_all(c.P[k].a, 12)) PSND_FAIL(PSND_E_ARG, "loudness: the filter's powers are not finite (a pole far outside the unit circle)");
    const long long R = B % H, slots = piece_slots(H, R);
    const size_t rs = (size_t)N * C * spans;
    double *carry = static_cast<double *>(scratch);
    double *part = reinterpret_cast<double *>(static_cast<char *>(scratch) + pad16(rs * 4 * sizeof(double)));
    int *flag = reinterpret_cast<int *>(reinterpret_cast<char *>(part) + pad16(rs * (size_t)slots * sizeof(double)));
    const long long *len = reinterpret_cast<const long long *>(lengths);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)rs);
    if (spans > 1) {
        hipLaunchKernelGGL(loudness_carry_kernel, grid, dim3(LANES), 0, st, x, (long long)T, len, (int)C, (int)spans, c, carry);
        PSND_CHECK_LAUNCH("loudness (span carries)");
    }
    hipLaunchKernelGGL(loudness_energy_kernel, grid, dim3(LANES), 0, st, x, (long long)T, len, (int)C, (int)spans, c, (long long)H, R,
                       (const double *)carry, part, flag);
    PSND_CHECK_LAUNCH("loudness (piece energies)");
    const Geo g = {(long long)T, (long long)B, (long long)H, R, (long long)psnd_loudness_blocks(T, B, H), (int)C, (int)spans};
    hipLaunchKernelGGL(loudness_final_kernel, dim3((unsigned)N), dim3(LANES), 0, st, len, g, G, pow(10.0, (-70.0 + 0.691) / 10.0), target, (const double *)part,
                       (const int *)flag,
                       lufs, blocks, gain);
    PSND_CHECK_LAUNCH("loudness (gates)");
    return PSND_OK;
}

extern "C" int psnd_row_level(const float *x, int64_t N, int64_t C, int64_t T, const int64_t *lengths, int of_peak, double target,
                              float *rms_db, float *peak_db, float *gain, void *stream) {
    if (C < 1) PSND_FAIL(PSND_E_ARG, "row_level: C=%lld", (long long)C);
    if (N < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "row_level: N=%lld T=%lld", (long long)N, (long long)T);
    if (of_peak != 0 && of_peak != 1) PSND_FAIL(PSND_E_ARG, "row_level: of_peak=%d", of_peak);
    if (!isfinite(target)) PSND_FAIL(PSND_E_ARG, "row_level: target is not finite");
    if (N == 0) return PSND_OK;
    if ((!x && T > 0) || (!rms_db && !peak_db && !gain)) PSND_FAIL(PSND_E_ARG, "row_level: null pointer");
    if (N > 0x7fffffff / C) PSND_FAIL(PSND_E_SHAPE, "row_level: N=%lld C=%lld is more than 2^31 - 1 rows", (long long)N, (long long)C);
    hipLaunchKernelGGL(row_level_kernel, dim3((unsigned)N), dim3(LV_LANES), 0, static_cast<hipStream_t>(stream), x, (long long)T,
                       reinterpret_cast<const long long *>(lengths), (int)C, of_peak, target, rms_db, peak_db, gain);
    PSND_CHECK_LAUNCH("row_level");
    return PSND_OK;
}

extern "C" int psnd_gain_rows(const float *x, int64_t N, int64_t C, int64_t T, const int64_t *lengths, const float *gain, float *y,
                              void *stream) {
    if (C < 1) PSND_FAIL(PSND_E_ARG, "gain_rows: C=%lld", (long long)C);
    if (N < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "gain_rows: N=%lld T=%lld", (long long)N, (long long)T);
    if (N == 0 || T == 0) return PSND_OK;
    if (!x || !y || !gain) PSND_FAIL(PSND_E_ARG, "gain_rows: null pointer");
    const long long chunks = (T + GAIN_PER - 1) / GAIN_PER;
    if (N > 0x7fffffff / C || N * C > 0x7fffffff / chunks)
        PSND_FAIL(PSND_E_SHAPE, "gain_rows: N=%lld C=%lld T=%lld is more than 2^31 - 1 workgroups", (long long)N, (long long)C, (long long)T);
    hipLaunchKernelGGL(gain_rows_kernel, dim3((unsigned)(N * C * chunks)), dim3(LANES), 0, static_cast<hipStream_t>(stream), x, (long long)T,
                       reinterpret_cast<const long long *>(lengths), (int)C, (int)chunks, gain, y);
    PSND_CHECK_LAUNCH("gain_rows");
    return PSND_OK;
}
