// probe: does v_mfma_f32_32x32x16_bf16 sum over k identically whichever operand carries which matrix?  One wave accumulates 48 units of
// random bf16 fragments into one accumulator, once as mfma(a, b) and once as mfma(b, a); the second result is the transpose of the first
// if and only if the hardware's order of summation does not depend on the operand slot.  Prints the count of differing 32-bit words
// (0 = the operand swap of psnd_conv_chain.hip is bit-exact).  hipcc --offload-arch=gfx950 -O2 probe_mfma_swap.hip -o probe_mfma_swap
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
constexpr int UNITS = 48;

// frag[u][lane] = 8 bf16: row / col `lane & 31`, k = 8 (lane >> 5) + j of unit u - the same lane map for both operands
__global__ void k(const bf16x8 *fa, const bf16x8 *fb, float *d_ab, float *d_ba) {
    const int l = threadIdx.x, li = l & 31, kg = l >> 5;
    f32x16 ab, ba;
    for (int q = 0; q < 16; ++q) ab[q] = 0.f, ba[q] = 0.f;
    for (int u = 0; u < UNITS; ++u) {
        const bf16x8 a = fa[u * 64 + l], b = fb[u * 64 + l];
        ab = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, ab, 0, 0, 0);
        ba = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, a, ba, 0, 0, 0);
    }
    // D[i][j]: lane holds column j = li, rows i = (q & 3) + 8 (q >> 2) + 4 kg
    for (int q = 0; q < 16; ++q) {
        const int i = (q & 3) + 8 * (q >> 2) + 4 * kg;
        d_ab[i * 32 + li] = ab[q];
        d_ba[i * 32 + li] = ba[q];
    }
}

static unsigned lcg(unsigned &s) { return s = s * 1664525u + 1013904223u; }
// a finite bf16 with a random sign, 7 random mantissa bits and a magnitude spread over 2^-6 ... 2^2 (sums that round at every step)
static unsigned short rnd_bf16(unsigned &s) {
    const unsigned r = lcg(s) >> 8;
    return (unsigned short)(((r & 1) << 15) | ((121 + (r >> 1) % 9) << 7) | ((r >> 8) & 0x7f));
}

int main() {
    const size_t nfrag = (size_t)UNITS * 64 * 8;
    unsigned short *ha = (unsigned short *)malloc(2 * nfrag), *hb = (unsigned short *)malloc(2 * nfrag);
    float h_ab[1024], h_ba[1024];
    bf16x8 *da, *db;
    float *d_ab, *d_ba;
    if (hipMalloc(&da, 2 * nfrag) != hipSuccess || hipMalloc(&db, 2 * nfrag) != hipSuccess || hipMalloc(&d_ab, sizeof(h_ab)) != hipSuccess ||
        hipMalloc(&d_ba, sizeof(h_ba)) != hipSuccess) {
        printf("hipMalloc failed\n");
        return 2;
    }
    long total = 0;
    for (unsigned seed = 1; seed <= 8; ++seed) {
        unsigned s = seed * 2654435761u;
        for (size_t i = 0; i < nfrag; ++i) ha[i] = rnd_bf16(s), hb[i] = rnd_bf16(s);
        hipMemcpy(da, ha, 2 * nfrag, hipMemcpyHostToDevice);
        hipMemcpy(db, hb, 2 * nfrag, hipMemcpyHostToDevice);
        hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, da, db, d_ab, d_ba);
        if (hipMemcpy(h_ab, d_ab, sizeof(h_ab), hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(h_ba, d_ba, sizeof(h_ba), hipMemcpyDeviceToHost) != hipSuccess) {
            printf("launch failed: %s\n", hipGetErrorString(hipGetLastError()));
            return 2;
        }
        int diff = 0, zero = 0;
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                diff += memcmp(&h_ab[i * 32 + j], &h_ba[j * 32 + i], 4) != 0;
                zero += h_ab[i * 32 + j] == 0.f;
            }
        printf("seed %u: %d of 1024 words differ between mfma(a, b) and mfma(b, a)^T (%d zeros, sample %.9g)\n", seed, diff, zero, h_ab[33]);
        total += diff;
    }
    printf("differing words: %ld\n", total);
    return total == 0 ? 0 : 1;
}
