// psnd_silence.hip - silent ranges per row of an (N, T) fp32 tensor on gfx950: the reference's utils/silence.py detect_silence (:25-80), which
// runs one x.dot(x) per window start in a Python loop on the host.  The definition is in include/psnd.h: window starts 0, s, 2s, ... and the
// last one T_r - L, a window silent iff its energy E <= theta and it holds no non-finite sample, silent starts merged into ranges in order.
//
// The energy of a window is NOT a difference of two row-long prefix sums: behind a loud passage the prefix is large and a quiet window's
// energy drowns in its rounding (2^20 samples, amplitude 1 then 1e-5, L = 10: off by up to 64 % in float64).  Prefixes restart at every block
// of BLK = 1024 samples, and a window is the tail of its first block + the totals of the whole blocks between + the head of its last block:
// three non-negative parts, each rounded relative to at most BLK + L terms of the window's own neighbourhood (1.4e-13 on that row).
//
// Three launches; no workgroup waits on another inside one, no atomics, no spinning (the rule of psnd_lfilter.hip):
//   A  prefix_kernel   one workgroup of 256 lanes per block of a row, four samples per lane by one 16-byte load (dword-aligned: a row may
//                      start on any 4-byte boundary; single dwords at the row's end).  x^2 in fp64, inclusive scan lane -> wave (shuffles)
//                      -> workgroup (LDS); the same scan in int32 over the count of non-finite samples, which enter the sum as 0.
//                      8 + 4 bytes of scratch per sample.  Blocks behind the row's length are neither written nor read.
//   B  decide_kernel   one lane per start: the decomposition above for E and for the non-finite count, one byte per start.  The flag rows
//                      are padded to a multiple of 16 starts and the padding is written as 0, so C loads 16 bytes per lane.
//   C  ranges_kernel   one workgroup per row, chunks of 256 x 16 starts.  A lane holds 16 flags as a bit mask.  The previous silent start
//                      p of a lane's first flag is an exclusive prefix maximum over the lanes' last silent starts; with p a lane applies the
//                      sequential rule to the starts of its runs of set bits (a silent start behind a silent grid neighbour never opens a
//                      range) and counts range heads; ordinals are an exclusive prefix sum of those counts; a second walk writes.  Inside
//                      a wave both scans are ballots: starts ascend with the lane, so the prefix maximum is the last silent start of the
//                      nearest lane below that has one, and the head counts (at most 9) are summed bit by bit with popcounts.  A head of
//                      ordinal r > 0 writes the end of range r - 1 (p + L) next to its own start; the last end, count and the -1 fill
//                      follow the walk.  Two barriers per chunk, on LDS alone (lds_barrier), so that the next chunk's flags, loaded
//                      before this one's are walked, stay in flight; the LDS words of the max scan are rewritten only behind the sum
//                      scan's barrier and the other way round.
// Every store into `ranges` is guarded by r < cap: the host checks cap >= psnd_silence_cap(T, L), which the definition never exceeds.
#include "psnd_common.h"

namespace {

constexpr int LANES = 256;
constexpr int WAVES = LANES / 64;
constexpr int BLK = PSND_SILENCE_BLOCK;
constexpr int PER = BLK / LANES;                        // samples per lane in A
constexpr int FPL = 16;                                 // flags per lane in C
constexpr int CHUNK = LANES * FPL;
static_assert(PER == 4, "A loads one f32x4 per lane");

__host__ __device__ inline long long n_starts(long long T, long long L, long long s) {
    if (T < L || T <= 0) return 0;
    const long long d = T - L;
    return d / s + 1 + (d % s != 0);
}
__host__ __device__ inline long long pad16(long long v) { return (v + 15) & ~15ll; }

__device__ __forceinline__ long long row_len(const long long *lengths, long long row, long long T) {
    if (!lengths) return T;
    const long long v = lengths[row];
    return v < 0 ? 0 : (v > T ? T : v);
}

// ---- A ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void prefix_kernel(const float *__restrict__ x, long long T, const long long *__restrict__ lengths,
                                                       int nblk, double *__restrict__ P, int *__restrict__ C) {
    __shared__ double wsum[WAVES];
    __shared__ int wcnt[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long row = blockIdx.x / nblk;
    const long long t0 = (long long)(blockIdx.x % nblk) * BLK;
    const long long len = row_len(lengths, row, T);
    if (t0 >= len) return;                              // the whole workgroup: nothing behind the row's length is read
    const float *xr = x + (size_t)row * T;
    const long long t = t0 + PER * tid;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (t + 3 < len) {
        v = *reinterpret_cast<const f32x4_u *>(xr + t);
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (t + k < len) v[k] = xr[t + k];
    }
    double q[PER];
    int c[PER];
    double run = 0.0;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const bool bad = (__float_as_uint(v[k]) & 0x7f800000u) == 0x7f800000u;
        const double d = bad ? 0.0 : (double)v[k];
        run += d * d;
        cnt += bad;
        q[k] = run;
        c[k] = cnt;
    }
    double si = run;                                    // inclusive scan of the lane totals over the wave
    int ci = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double so = __shfl_up(si, d, 64);
        const int co = __shfl_up(ci, d, 64);
        if (lane >= d) si += so, ci += co;
    }
    if (lane == 63) wsum[w] = si, wcnt[w] = ci;
    __syncthreads();
    double base = 0.0;
    int cbase = 0;
    for (int k = 0; k < w; ++k) base += wsum[k], cbase += wcnt[k];
    base += si - run;                                   // what lies before this lane
    cbase += ci - cnt;
    double *Pr = P + (size_t)row * T + t;
    int *Cr = C + (size_t)row * T + t;
#pragma unroll
    for (int k = 0; k < PER; ++k)
        if (t + k < len) Pr[k] = base + q[k], Cr[k] = cbase + c[k];
}

// ---- B ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void decide_kernel(const long long *__restrict__ lengths, long long T, long long L, long long s,
                                                       double theta, const double *__restrict__ P, const int *__restrict__ C,
                                                       unsigned char *__restrict__ flags, long long Sp, int jblocks) {
    const long long row = blockIdx.x / jblocks;
    const long long j = (long long)(blockIdx.x % jblocks) * LANES + threadIdx.x;
    if (j >= Sp) return;
    const long long len = row_len(lengths, row, T);
    const long long n = n_starts(len, L, s);
    unsigned char f = 0;
    if (j < n) {
        const long long i = min(j * s, len - L), e = i + L - 1;         // j s <= len - L + s: no overflow, s <= T + 1
        const long long b0 = i / BLK, b1 = e / BLK;
        const double *Pr = P + (size_t)row * T;
        const int *Cr = C + (size_t)row * T;
        const bool at_block = i % BLK == 0;
        const double before = at_block ? 0.0 : Pr[i - 1];
        const int cbefore = at_block ? 0 : Cr[i - 1];
        double E;
        int bad;
        if (b0 == b1) {
            E = Pr[e] - before;
            bad = Cr[e] - cbefore;
        } else {
            const long long last = b0 * BLK + BLK - 1;
            E = Pr[last] - before;
            bad = Cr[last] - cbefore;
            for (long long b = b0 + 1; b < b1; ++b) {                   // at most L / BLK + 1 whole blocks
                E += Pr[b * BLK + BLK - 1];
                bad += Cr[b * BLK + BLK - 1];
            }
            E += Pr[e];
            bad += Cr[e];
        }
        f = bad == 0 && E <= theta;
    }
    flags[(size_t)row * Sp + j] = f;
}

// A barrier for words exchanged through LDS alone: the LDS writes before it have landed, loads from global memory stay in flight across it
// (__syncthreads() waits for those as well, and would put the load of the next chunk's flags back in front of every barrier of ranges_kernel)
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// ---- C ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void ranges_kernel(const long long *__restrict__ lengths, long long T, long long L, long long s,
                                                       const unsigned char *__restrict__ flags, long long Sp, int *__restrict__ count,
                                                       long long *__restrict__ ranges, long long cap) {
    __shared__ long long wmax[WAVES];
    __shared__ int whead[WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long row = blockIdx.x;
    const long long len = row_len(lengths, row, T);
    const long long n = n_starts(len, L, s);
    const long long last_start = len - L;
    const unsigned char *fr = flags + (size_t)row * Sp;
    long long *R = ranges + (size_t)row * cap * 2;
    long long p_carry = -1;                             // the last silent start so far, -1: none
    long long ord_carry = 0;                            // ranges opened so far
    const bool off_grid = n > 0 && last_start % s != 0;  // the last start is no grid point: the one start whose grid neighbour is not s away
    // 16 flag bytes of a lane (j0 % 16 == 0 and Sp % 16 == 0: they lie inside the row, its padding is 0); the next chunk's are in flight
    // while this one is walked
    auto load = [&](long long j) -> u32x4 {             // no branch: behind the row's starts the row's first 16 bytes are read and dropped
        const u32x4 v = *reinterpret_cast<const u32x4 *>(fr + (j < n ? j : 0));
        const unsigned keep = j < n ? ~0u : 0u;
        return u32x4{v[0] & keep, v[1] & keep, v[2] & keep, v[3] & keep};
    };
    auto start_of = [&](long long j) -> long long { return min(j * s, last_start); };
    u32x4 cur = {0u, 0u, 0u, 0u};
    if (n > 0) cur = load((long long)FPL * tid);        // a row without starts may have no flag bytes at all
    for (long long c0 = 0; c0 < n; c0 += CHUNK) {
        const long long j0 = c0 + (long long)FPL * tid;
        const u32x4 nxt = load(j0 + CHUNK);
        unsigned m = 0;                                 // bytes of 0 / 1 -> one bit each: byte k of a word times 2^(24 - 7k) lands on bit 24 + k
#pragma unroll
        for (int k = 0; k < 4; ++k) m |= (((cur[k] & 0x01010101u) * 0x01020408u) >> 24) << (4 * k);
        cur = nxt;
        // the previous silent start of every lane: exclusive prefix maximum of the lanes' last silent starts.  Starts ascend with the lane,
        // so it is the last silent start of the nearest lane below that has one: a ballot and one cross-lane read, no scan
        const unsigned long long below_me = (1ull << lane) - 1ull;
        const unsigned long long any = __ballot(m != 0);
        const unsigned long long lower = any & below_me;
        const int last_local = m ? FPL * tid + (31 - __builtin_clz(m)) : 0;             // index inside the chunk
        const int from = __shfl(last_local, lower ? 63 - __builtin_clzll(lower) : 0, 64);
        long long p_in = lower ? start_of(c0 + from) : -1;
        if (any ? lane == 63 - __builtin_clzll(any) : lane == 0) wmax[w] = any ? start_of(c0 + last_local) : -1;
        lds_barrier();
        p_in = max(p_in, p_carry);
#pragma unroll
        for (int k = 0; k < WAVES; ++k) {               // read here: wmax is rewritten behind the next barrier
            const long long v = wmax[k];
            p_in = max(p_in, k < w ? v : -1);
            p_carry = max(p_carry, v);
        }
        // A silent start whose left neighbour on the grid is silent too has k = p + s: no head.  Heads are among the starts of the runs of
        // set bits, and the last start of the row where it lies off the grid; p of such a bit is the set bit below it, or p_in.
        unsigned cand = m & ~(m << 1);
        if (off_grid && n - 1 >= j0 && n - 1 < j0 + FPL) cand |= m & (1u << (int)(n - 1 - j0));
        auto walk = [&](auto &&on_head) {
            for (unsigned cc = cand; cc; cc &= cc - 1) {
                const int b = __builtin_ctz(cc);
                const unsigned below = m & ((1u << b) - 1u);
                const long long p = below ? start_of(j0 + (31 - __builtin_clz(below))) : p_in;
                const long long i = start_of(j0 + b);
                if (p < 0 || (i != p + s && i > p + L)) on_head(i, p);
            }
        };
        int heads = 0;
        walk([&](long long, long long) { ++heads; });
        // at most 9 heads per lane (eight runs in 16 bits and the off-grid last start): the exclusive sum over the wave from four ballots
        int before = 0, total = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned long long has = __ballot((heads >> b) & 1);
            before += __builtin_popcountll(has & below_me) << b;
            total += __builtin_popcountll(has) << b;
        }
        if (lane == 0) whead[w] = total;
        lds_barrier();
        long long ord = ord_carry + before;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) {
            const int v = whead[k];
            ord += k < w ? v : 0;
            ord_carry += v;
        }
        // a head writes its start and the end of the range before
        if (heads)
            walk([&](long long i, long long p) {
                if (ord < cap) R[2 * ord] = i;
                if (ord > 0 && ord - 1 < cap) R[2 * (ord - 1) + 1] = p + L;
                ++ord;
            });
    }
    if (tid == 0) {
        count[row] = (int)ord_carry;
        if (ord_carry > 0 && ord_carry - 1 < cap) R[2 * (ord_carry - 1) + 1] = p_carry + L;
    }
    for (long long r = ord_carry + tid; r < cap; r += LANES) R[2 * r] = -1, R[2 * r + 1] = -1;
}

}  // namespace

extern "C" int64_t psnd_silence_cap(int64_t T, int64_t L) {
    if (L < 1 || T < L) return 0;
    return (T - L) / (L + 1) + 1;
}

extern "C" int64_t psnd_silence_starts(int64_t T, int64_t L, int64_t s) {
    if (L < 1 || s < 1) return 0;
    return n_starts(T, L, s);
}

extern "C" size_t psnd_silence_scratch_bytes(int64_t N, int64_t T, int64_t L, int64_t s) {
    if (N <= 0 || T <= 0 || L < 1 || s < 1) return 0;
    return (size_t)pad16((long long)N * T * 12) + (size_t)N * (size_t)pad16(n_starts(T, L, s));
}

extern "C" int psnd_silence_ranges(const float *x, int64_t N, int64_t T, const int64_t *lengths, int64_t L, int64_t s, double theta,
                                   void *scratch, int32_t *count, int64_t *ranges, int64_t cap, void *stream) {
    if (L < 1 || s < 1) PSND_FAIL(PSND_E_ARG, "silence: L=%lld s=%lld (window and step are at least one sample)", (long long)L, (long long)s);
    if (N < 0 || T < 0) PSND_FAIL(PSND_E_ARG, "silence: N=%lld T=%lld", (long long)N, (long long)T);
    if (theta != theta) PSND_FAIL(PSND_E_ARG, "silence: theta is NaN");
    if (cap < psnd_silence_cap(T, L))
        PSND_FAIL(PSND_E_ARG, "silence: cap=%lld, a row of T=%lld with L=%lld can hold psnd_silence_cap = %lld ranges", (long long)cap,
                  (long long)T, (long long)L, (long long)psnd_silence_cap(T, L));
    if (N == 0 || T == 0) return PSND_OK;
    if (!x || !count || (!ranges && cap > 0)) PSND_FAIL(PSND_E_ARG, "silence: null pointer");
    if (s > T) s = T + 1;                               // the same starts and the same merges for every step beyond the row
    const long long S = n_starts(T, L, s), Sp = pad16(S);
    if (S > 0 && !scratch) PSND_FAIL(PSND_E_ARG, "silence: null scratch");
    if ((uintptr_t)scratch % 16) PSND_FAIL(PSND_E_ARG, "silence: scratch must be 16-byte aligned");
    const long long nblk = (T + BLK - 1) / BLK, jblocks = (Sp + LANES - 1) / LANES;
    if (N > 0x7fffffff || N * nblk > 0x7fffffff || N * jblocks > 0x7fffffff)
        PSND_FAIL(PSND_E_SHAPE, "silence: N=%lld T=%lld is more than 2^31 - 1 workgroups", (long long)N, (long long)T);
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *P = static_cast<double *>(scratch);
    int *C = reinterpret_cast<int *>(P + (size_t)N * T);
    unsigned char *flags = static_cast<unsigned char *>(scratch) + pad16((long long)N * T * 12);
    const long long *len = reinterpret_cast<const long long *>(lengths);
    if (S > 0) {
        hipLaunchKernelGGL(prefix_kernel, dim3((unsigned)(N * nblk)), dim3(LANES), 0, st, x, (long long)T, len, (int)nblk, P, C);
        PSND_CHECK_LAUNCH("silence prefix");
        hipLaunchKernelGGL(decide_kernel, dim3((unsigned)(N * jblocks)), dim3(LANES), 0, st, len, (long long)T, (long long)L, (long long)s,
                           theta, (const double *)P, (const int *)C, flags, Sp, (int)jblocks);
        PSND_CHECK_LAUNCH("silence decide");
    }
    hipLaunchKernelGGL(ranges_kernel, dim3((unsigned)N), dim3(LANES), 0, st, len, (long long)T, (long long)L, (long long)s,
                       (const unsigned char *)flags, Sp, (int *)count, reinterpret_cast<long long *>(ranges), (long long)cap);
    PSND_CHECK_LAUNCH("silence ranges");
    return PSND_OK;
}
