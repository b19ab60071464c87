// psnd_span_stage.h - staging of a span of one fp32 row through LDS for the kernels that walk time sequentially per lane (psnd_sound.hip,
// psnd_lfilter.hip): 16-byte global loads and stores by a workgroup of STAGE_LANES threads, zeros outside the row, and the pitched image.
//
// Lanes walk LDS with a stride of one chunk of 32 samples, so the image is pitched: sample i sits at word i + i / 32, i.e. lane l starts at
// word 33 l + const and the 32 lanes of an LDS access group hit 32 different banks.  No lane walks global memory.
#pragma once
#include "psnd_common.h"

constexpr int STAGE_LANES = 256;

__device__ __forceinline__ int pitched(int i) { return i + (i >> 5); }

// s[pos(i)] = src[t0 + i] for i in [0, n), n % 4 == 0, zeros where t0 + i is outside [0, T).  PITCH: pitched image, else plain.
template <bool PITCH>
__device__ __forceinline__ void stage_in(float *s, const float *row, long long T, long long t0, int n) {
    for (int i = 4 * threadIdx.x; i < n; i += 4 * STAGE_LANES) {
        const long long t = t0 + i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t + 3 < T) {
            v = *reinterpret_cast<const f32x4_u *>(row + t);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t + k >= 0 && t + k < T) v[k] = row[t + k];
        }
        const int p = PITCH ? pitched(i) : i;           // i % 4 == 0: the four words stay inside one group of 32
#pragma unroll
        for (int k = 0; k < 4; ++k) s[p + k] = v[k];
    }
}
// dst[t0 + i] = s[pos(i0 + i)] for i in [0, n), n % 4 == 0, i0 % 4 == 0, where t0 + i < T   (t0 >= 0)
template <bool PITCH>
__device__ __forceinline__ void stage_out(const float *s, int i0, float *row, long long T, long long t0, int n) {
    for (int i = 4 * threadIdx.x; i < n; i += 4 * STAGE_LANES) {
        const long long t = t0 + i;
        if (t >= T) break;
        const int p = PITCH ? pitched(i0 + i) : i0 + i;
        f32x4 v;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = s[p + k];
        if (t + 3 < T) {
            *reinterpret_cast<f32x4_u *>(row + t) = v;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (t + k < T) row[t + k] = v[k];
        }
    }
}
