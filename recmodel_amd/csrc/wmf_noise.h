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
//
// The noise of the posterior draws (wmf_posterior.hip): a standard normal variate as a PURE FUNCTION of (seed, stream, draw, component),
// so that draw s of a row cannot depend on the number of draws asked for, the row's position or the other rows of the launch.  One text
// for the draw kernel and for the diagnostic entry wmf_posterior_noise; tests/posterior_ref.py restates it.
//
//   a  = mix(seed + 0x9E3779B97F4A7C15 * (stream + 1))             the row's prefix above
//   h  = mix(a + 0x9E3779B97F4A7C15 * (2^32 * (draw + 1) + component + 1))      draw, component zero-extended from 32 bits, draw < 2^31
//   k1 = h >> 41;  k2 = (h >> 18) & 0x7FFFFF                       23 bits each, disjoint bits of h
//   u1 = (2 k1 + 1) * 2^-24;  t = (2 k2 + 1) * 2^-23               exact in float32: u1 in (0, 1), t in (0, 2)
//   xi = sqrtf(-2 logf(u1)) * cospif(t)                            Box-Muller; the accurate logf, sqrtf and cospif
//
// The keys 2^32 (draw + 1) + component + 1 are at least 2^32 + 1; the item keys of the Gumbel noise are at most 2^32: one (seed, stream)
// serves a sampled list and a draw without a shared hash input.  The tail is CUT OFF: |xi| <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.768,
// a normal variate beyond it (probability 8e-9) is never drawn; t is never 1/2 or 3/2, so xi is never an exact zero of the cosine.
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
// the hash of (row prefix a, draw, component): k1 = h >> 41, k2 = (h >> 18) & 0x7FFFFF
__host__ __device__ __forceinline__ uint64_t wmf_noise_normal_h(uint64_t a, int32_t draw, int32_t component) {
    return wmf_noise_mix(a + WMF_NOISE_GOLDEN * ((((uint64_t)(uint32_t)draw + 1ull) << 32) + (uint64_t)(uint32_t)component + 1ull));
}
__device__ __forceinline__ float wmf_noise_normal(uint64_t h) {
    const float u1 = (float)(2u * (uint32_t)(h >> 41) + 1u) * 0x1p-24f;             // exact: an odd 24-bit integer
    const float t = (float)(2u * ((uint32_t)(h >> 18) & 0x7FFFFFu) + 1u) * 0x1p-23f;
    return sqrtf(-2.f * logf(u1)) * cospif(t);
}
