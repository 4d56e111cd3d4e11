// The gather helpers that the one-workgroup-per-row kernels with an on-the-fly whitened history share (wmf_explain.hip,
// wmf_foldin.hip): 256 threads as 16 groups of 16 lanes, a chunk of EX_CHUNK stored entries at a time.  Pure functions of their
// arguments: fixed summation orders, no atomics.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#define EX_CHUNK 8                          /* stored entries gathered and whitened at a time */

// sum over the 16 lanes of a group, the same bits on every lane
__device__ __forceinline__ float ex_sum16(float v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// out[e][b] = sum over a <= b of raw[e][a] W[a][b] for the 8 rows of raw (LDS, f floats each), a thread per column b; the rows
// from cnt on are written as zero
__device__ __forceinline__ void ex_whiten8(const float* raw, float* out, const float* __restrict__ W, int f, int ld, int cnt) {
    for (int b = threadIdx.x; b < f; b += 256) {
        float acc[EX_CHUNK];
#pragma unroll
        for (int e = 0; e < EX_CHUNK; ++e) acc[e] = 0.f;
        for (int a = 0; a <= b; ++a) {
            const float wv = W[(int64_t)a * ld + b];
#pragma unroll
            for (int e = 0; e < EX_CHUNK; ++e) acc[e] = fmaf(raw[e * f + a], wv, acc[e]);
        }
#pragma unroll
        for (int e = 0; e < EX_CHUNK; ++e) out[e * f + b] = e < cnt ? acc[e] : 0.f;
    }
}

// row `src` of the fixed side with column 0 read as 1 (bias), or zeros (src == NULL), into f floats of LDS: the 16 lanes of a group
__device__ __forceinline__ void ex_load_row(const float* __restrict__ src, float* dst, int f, int bias, int g) {
    for (int a = g; a < f; a += 16) dst[a] = !src ? 0.f : (bias && a == 0) ? 1.f : src[a];
}
