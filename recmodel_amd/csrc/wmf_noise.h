// The noise of the sampled top-n (gfx950): a standard Gumbel variate as a PURE FUNCTION of (seed, stream, item), so that a draw cannot
// depend on the batch position, the batch's composition, the slice count, the grid or the form of the filter.  One text for the
// scan's perturbing epilogue (wmf_sample.hip) and for the diagnostic entry wmf_sample_noise; tests/sample_ref.py restates it.
//
//   mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31      (uint64, wrapping)
//   a = mix(seed + 0x9E3779B97F4A7C15 * (stream + 1))             once per row
//   h = mix(a    + 0x9E3779B97F4A7C15 * (item   + 1))             item zero-extended from its 32-bit id
//   k = h >> 41                                                   23 bits
//   u = (2 k + 1) * 2^-24                                         exact in float32, in [2^-24, 1 - 2^-24]
//   g = -logf(-logf(u))                                           the accurate logf (this file is never compiled with fast-math)
//
// The tail is CUT OFF: g lies in [-2.8116, 16.6356] (k = 0 and k = 2^23 - 1), a Gumbel variate beyond either end is never drawn, and
// relative probabilities below about e^-16 are not resolved.  g is clamped to WMF_SAMPLE_G_MAX, the float32 value of g at k = 2^23 - 1,
// so that no last bit of a logf can put a draw above the bound the scan's skip test stands on (wmf_sample.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/wmf_hip.h"                                 /* WMF_SAMPLE_G_MAX = 16.635532: -logf(-logf(1 - 2^-24)) */

#define WMF_NOISE_GOLDEN 0x9E3779B97F4A7C15ull

__host__ __device__ __forceinline__ uint64_t wmf_noise_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// the row's prefix of the hash
__host__ __device__ __forceinline__ uint64_t wmf_noise_row(uint64_t seed, uint64_t stream) {
    return wmf_noise_mix(seed + WMF_NOISE_GOLDEN * (stream + 1ull));
}
// the 23 bits of (row prefix a, item)
__host__ __device__ __forceinline__ uint32_t wmf_noise_k(uint64_t a, int32_t item) {
    return (uint32_t)(wmf_noise_mix(a + WMF_NOISE_GOLDEN * ((uint64_t)(uint32_t)item + 1ull)) >> 41);
}
__device__ __forceinline__ float wmf_noise_g(uint32_t k) {
    const float u = (float)(2u * k + 1u) * 0x1p-24f;               // exact: an odd 24-bit integer
    return fminf(-logf(-logf(u)), WMF_SAMPLE_G_MAX);
}
