// The posterior of a folded-in row (gfx950): in the probabilistic reading of the row system of wmf_foldin.hip,
//     x_u ~ N(A_u^-1 b_u, A_u^-1),      A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T,
// and in whitened coordinates q = y~ W_white, where A_u^-1 = W_white (I + E_u)^-1 W_white^T and I + E_u = L L^T,
//     a draw          x~_s      = W_white L^-T (c + sigma xi_s),       c = L^-1 b, xi_s standard normal       (posterior_draw_kernel)
//     a score's law   var(u, i) = z_i . z_i,  mean(u, i) = z_i . c + beta_i,       z_i = L^-1 q_i             (posterior_score_kernel)
// Definitions: include/wmf_hip.h, wmf_posterior_draw_rows / wmf_posterior_score_rows; derivation and LDS budget: DESIGN.md section 5.
//
// One 256-thread workgroup per row, grid-stride over the rows; everything of a row lives in LDS (dynamic, sized by f):
//     tri   packed lower triangle of f + 1 rows as in wmf_foldin.hip: rows 0 .. f - 1 are I + E_u, then L; row f is b, then c
//     slot  16 vectors of f floats: the raw and the whitened chunk of 8 entries while E_u is accumulated and the scaled pivot column
//           of the factorisation (the fold-in's raw and qb), then the 16 right-hand sides of a pass
//     stage 8 rows of f floats, the score kernel only: the raw target rows of half a pass
//     dinv  1 / L[k][k]
// Phases 1 and 2 (po_factor_row) are those of wmf_foldin.hip, operation for operation: the gather in chunks of 8 entries, w_e q q^T
// and (w_e + 1) q entry by entry in stored order, the right-looking Cholesky that carries b as row f.  Then, 16 at a time with a
// 16-lane group per right-hand side (wmf_explain.hip's pattern for its slots): the draw kernel solves L^T g = c + sigma xi_s without
// touching c and multiplies by W_white; the score kernel gathers and whitens 16 targets, solves L z = q and takes two dot products.
// A pass of one draw takes the whole workgroup for the substitution instead, as the fold-in does: every element sees the same
// operations in the same order either way, so draw s has the same bits in both, and at sigma == 0 they are the fold-in's.
// No floating-point atomics, fixed orders everywhere: a row's arithmetic depends on nothing but the row (and its stream), a slot's on
// nothing but the slot (all 16 are always computed: empty ones hold 0).
#include <float.h>
#include <math.h>
#include "wmf_common.h"
#include "wmf_internal.h"
#include "wmf_noise.h"
#include "wmf_rowgather.h"                  /* EX_CHUNK, ex_sum16, ex_whiten8, ex_load_row: shared with wmf_explain.hip, wmf_foldin.hip */

#define PO_SLOTS 16                         /* right-hand sides of a pass: one 16-lane group each */
#define WMF_POSTERIOR_MAX_BLOCKS 1024
#define WMF_POSTERIOR_WS_BYTES 256
#define WMF_POSTERIOR_NOISE_GRID 1024

static_assert(PO_SLOTS == 2 * EX_CHUNK, "the 16 slots are the fold-in's raw and whitened chunk");

// floats of a row's LDS.  The one budget of each kernel: the launch and the kernel's ceiling both come from here.
__host__ __device__ static inline int po_tri_floats(int f) { return (f + 1) * (f + 2) / 2; }
static inline size_t po_draw_lds_bytes(int f) { return (size_t)(po_tri_floats(f) + (PO_SLOTS + 1) * f) * sizeof(float); }
static inline size_t po_score_lds_bytes(int f) { return (size_t)(po_tri_floats(f) + (PO_SLOTS + EX_CHUNK + 1) * f) * sizeof(float); }
static_assert((WMF_MAX_F + 1) * (WMF_MAX_F + 2) / 2 + (PO_SLOTS + EX_CHUNK + 1) * WMF_MAX_F <= 160 * 1024 / 4 - 64,
              "the row system of the widest model must fit the LDS of a CU");

// Phases 1 and 2 of a non-empty row: I + E_u and b into `tri`, then L and c = L^-1 b in their place and 1 / L[k][k] in dinv.  raw, qb:
// 8 f floats each (qb also holds the f + 1 floats of a pivot column: f >= 1).  False, for every thread alike, if a pivot is not positive
// and finite.  Ends on a barrier.
__device__ __forceinline__ bool po_factor_row(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                              const int32_t* __restrict__ indices, const float* __restrict__ vals, int64_t lo, int64_t hi,
                                              float* tri, float* raw, float* qb, float* dinv, float* s_w) {
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    float* bv = tri + f * (f + 1) / 2;
    for (int i = grp; i <= f; i += 16) {
        float* row = tri + i * (i + 1) / 2;
        for (int j = g; j <= i; j += 16) row[j] = (j == i && i < f) ? 1.f : 0.f;
    }
    for (int64_t c0 = lo; c0 < hi; c0 += EX_CHUNK) {
        const int cnt = hi - c0 < EX_CHUNK ? (int)(hi - c0) : EX_CHUNK;
        if (grp < EX_CHUNK) {
            const float* src = grp < cnt ? Y + (int64_t)indices[c0 + grp] * ld : nullptr;
            ex_load_row(src, raw + grp * f, f, bias, g);
            if (g == 0) s_w[grp] = src ? vals[c0 + grp] - (bias ? src[0] : 0.f) : 0.f;
        }
        __syncthreads();                                           // (also: the zeroed triangle, before the first chunk adds to it)
        ex_whiten8(raw, qb, W, f, ld, cnt);
        __syncthreads();
        for (int i = grp; i < f; i += 16) {
            float wq[EX_CHUNK];
#pragma unroll
            for (int e = 0; e < EX_CHUNK; ++e) wq[e] = s_w[e] * qb[e * f + i];
            float* row = tri + i * (i + 1) / 2;
            for (int j = g; j <= i; j += 16) {
                float s = row[j];
#pragma unroll
                for (int e = 0; e < EX_CHUNK; ++e) s = fmaf(wq[e], qb[e * f + j], s);
                row[j] = s;
            }
        }
        for (int a = tid; a < f; a += 256) {
            float s = bv[a];
            for (int e = 0; e < cnt; ++e) s = fmaf(s_w[e] + 1.f, qb[e * f + a], s);
            bv[a] = s;
        }
        __syncthreads();                                           // the next chunk overwrites raw, qb and s_w
    }
    // Cholesky of the f + 1 rows, right-looking: the pivot is the same LDS word for every thread, so the exit is uniform
    float* col = qb;
    for (int k = 0; k < f; ++k) {
        const float p = tri[k * (k + 1) / 2 + k];
        if (!(p > 0.f) || p > FLT_MAX) return false;
        const float r = 1.f / sqrtf(p);
        for (int i = k + 1 + tid; i <= f; i += 256) {
            float* e = tri + i * (i + 1) / 2 + k;
            const float v = *e * r;
            *e = v;
            col[i] = v;
        }
        if (tid == 0) dinv[k] = r;
        __syncthreads();
        for (int i = k + 1 + grp; i <= f; i += 16) {
            const float ci = -col[i];
            float* row = tri + i * (i + 1) / 2;
            const int last = i < f ? i : f - 1;                    // (row f has no diagonal)
            for (int j = k + 1 + g; j <= last; j += 16) row[j] = fmaf(ci, col[j], row[j]);
        }
        __syncthreads();
    }
    return true;
}

// ---- draws --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void posterior_draw_kernel(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                                             const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                             const float* __restrict__ vals, int64_t n, int n_draws, float sigma, uint64_t seed,
                                                             const uint64_t* __restrict__ row_stream, float* __restrict__ X_out,
                                                             int32_t* __restrict__ fail_count) {
    extern __shared__ float po_lds[];
    __shared__ float s_w[EX_CHUNK];
    float* tri = po_lds;
    float* slot = tri + po_tri_floats(f);                          // 16 f floats: raw (8 f) and qb (8 f) of phases 1 and 2
    float* dinv = slot + PO_SLOTS * f;
    const float* cv = tri + f * (f + 1) / 2;                       // row f of the triangle: c = L^-1 b, read by every pass
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    const float nan = __int_as_float(0x7fc00000);

    for (int64_t u = blockIdx.x; u < n; u += gridDim.x) {
        const int64_t lo = indptr[u], hi = indptr[u + 1];
        float* xo = X_out + u * n_draws * ld;                      // the n_draws rows of this row
        const bool empty = hi <= lo;
        if (empty && sigma == 0.f) {                               // the fold-in's zeros (wmf_model.py:274-276)
            for (int64_t x = tid; x < (int64_t)n_draws * ld; x += 256) xo[x] = 0.f;
            continue;                                              // (uniform; no LDS was touched)
        }
        // an empty row has I + E_u = I and c = 0: its draws are the prior's, W_white sigma xi
        const bool ok = empty || po_factor_row(Y, f, ld, bias, W, indices, vals, lo, hi, tri, slot, slot + EX_CHUNK * f, dinv, s_w);
        if (!ok) {
            for (int64_t x = tid; x < (int64_t)n_draws * ld; x += 256) xo[x] = (int)(x % ld) < f ? nan : 0.f;
            if (tid == 0) atomicAdd(fail_count, 1);
            __syncthreads();                                       // the next row of this workgroup rewrites the triangle
            continue;
        }
        const uint64_t a_row = wmf_noise_row(seed, row_stream ? row_stream[u] : (uint64_t)u);
        for (int s0 = 0; s0 < n_draws; s0 += PO_SLOTS) {
            const int cnt = n_draws - s0 < PO_SLOTS ? n_draws - s0 : PO_SLOTS;
            // the right-hand sides c + sigma xi_s (sigma == 0: c itself, no product -- a signed zero would differ); slots from cnt on: 0
            float* x = slot + grp * f;
            for (int i = g; i < f; i += 16) {
                float v = 0.f;
                if (grp < cnt) {
                    v = empty ? 0.f : cv[i];
                    if (sigma != 0.f) v = fmaf(sigma, wmf_noise_normal(wmf_noise_normal_h(a_row, s0 + grp, i)), v);
                }
                x[i] = v;
            }
            __syncthreads();
            // L^T g = x in place.  Step k: g_k = x_k / L_kk, then x_i -= L_ki g_k for i < k -- x_k is final once the steps above k are done
            if (empty) {
                // L = I: g = x
            } else if (cnt == 1) {                                 // one draw: the whole workgroup on slot 0, as wmf_foldin.hip
                float* x0 = slot;
                for (int k = f - 1; k >= 0; --k) {
                    const float zk = x0[k] * dinv[k];
                    const float* row = tri + k * (k + 1) / 2;
                    for (int i = tid; i < k; i += 256) x0[i] = fmaf(-row[i], zk, x0[i]);
                    __syncthreads();                               // every thread has read x0[k] and written its part of x0[0 .. k)
                    if (tid == 0) x0[k] = zk;                      // (read again only by the product below)
                }
            } else {
                for (int k = f - 1; k >= 0; --k) {
                    const float zk = x[k] * dinv[k];
                    const float* row = tri + k * (k + 1) / 2;
                    for (int i = g; i < k; i += 16) x[i] = fmaf(-row[i], zk, x[i]);
                    __syncthreads();                               // every lane has read x[k] and written its part of x[0 .. k)
                    if (g == 0) x[k] = zk;
                }
            }
            __syncthreads();
            // x~ = W g over b >= a, a group per component a and all 16 slots on every lane; the fold-in's order
            for (int a = grp; a < f; a += 16) {
                float acc[PO_SLOTS];
#pragma unroll
                for (int s = 0; s < PO_SLOTS; ++s) acc[s] = 0.f;
                for (int b = a + g; b < f; b += 16) {
                    const float wv = W[(int64_t)a * ld + b];
#pragma unroll
                    for (int s = 0; s < PO_SLOTS; ++s) acc[s] = fmaf(wv, slot[s * f + b], acc[s]);
                }
#pragma unroll
                for (int s = 0; s < PO_SLOTS; ++s) {
                    const float v = ex_sum16(acc[s]);
                    if (g == s && s < cnt) xo[(int64_t)(s0 + s) * ld + a] = v;
                }
            }
            for (int x2 = tid; x2 < cnt * (ld - f); x2 += 256) xo[(int64_t)(s0 + x2 / (ld - f)) * ld + f + x2 % (ld - f)] = 0.f;
            __syncthreads();                                       // the next pass, or the next row, rewrites the slots
        }
    }
}

// ---- the law of a score -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void posterior_score_kernel(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                                              const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                              const float* __restrict__ vals, int64_t n, const int32_t* __restrict__ targets,
                                                              int T, float* __restrict__ out_mean, float* __restrict__ out_var,
                                                              int32_t* __restrict__ fail_count) {
    extern __shared__ float po_lds[];
    __shared__ float s_w[EX_CHUNK], s_beta[PO_SLOTS];
    __shared__ int s_tgt[PO_SLOTS];
    float* tri = po_lds;
    float* slot = tri + po_tri_floats(f);
    float* stage = slot + PO_SLOTS * f;
    float* dinv = stage + EX_CHUNK * f;
    const float* cv = tri + f * (f + 1) / 2;
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    const float nan = __int_as_float(0x7fc00000);

    for (int64_t u = blockIdx.x; u < n; u += gridDim.x) {
        const int64_t lo = indptr[u], hi = indptr[u + 1];
        const bool empty = hi <= lo;                               // I + E_u = I and c = 0: z = q, var = |q|^2, mean = beta
        const bool ok = empty || po_factor_row(Y, f, ld, bias, W, indices, vals, lo, hi, tri, slot, slot + EX_CHUNK * f, dinv, s_w);
        if (!ok && tid == 0) atomicAdd(fail_count, 1);
        for (int t0 = 0; t0 < T; t0 += PO_SLOTS) {
            const int cnt = T - t0 < PO_SLOTS ? T - t0 : PO_SLOTS;
            if (tid < PO_SLOTS) {
                const int t = tid < cnt ? targets[u * T + t0 + tid] : -1;
                s_tgt[tid] = t;
                s_beta[tid] = (t >= 0 && bias) ? Y[(int64_t)t * ld] : 0.f;
            }
            __syncthreads();
            if (!ok) {
                if (tid < cnt) {
                    const float v = s_tgt[tid] >= 0 ? nan : 0.f;
                    if (out_mean) out_mean[u * T + t0 + tid] = v;
                    if (out_var) out_var[u * T + t0 + tid] = v;
                }
                __syncthreads();                                   // the next pass rewrites s_tgt
                continue;                                          // (uniform)
            }
            // q_i of the 16 slots (an empty slot: zeros), half a pass at a time
            for (int h = 0; h < PO_SLOTS / EX_CHUNK; ++h) {
                if (h * EX_CHUNK >= cnt) {
                    for (int x = tid; x < EX_CHUNK * f; x += 256) slot[h * EX_CHUNK * f + x] = 0.f;
                    continue;                                      // (uniform)
                }
                if (grp < EX_CHUNK) {
                    const int t = s_tgt[h * EX_CHUNK + grp];
                    ex_load_row(t >= 0 ? Y + (int64_t)t * ld : nullptr, stage + grp * f, f, bias, g);
                }
                __syncthreads();
                ex_whiten8(stage, slot + h * EX_CHUNK * f, W, f, ld, EX_CHUNK);
                __syncthreads();
            }
            __syncthreads();
            // L z = q in place: slot `grp` on the 16 lanes of group `grp`
            float* x = slot + grp * f;
            if (!empty) {
                for (int i = 0; i < f; ++i) {
                    const float* row = tri + i * (i + 1) / 2;
                    float s = 0.f;
                    for (int k = g; k < i; k += 16) s = fmaf(row[k], x[k], s);
                    s = ex_sum16(s);
                    if (g == 0) x[i] = (x[i] - s) * dinv[i];
                    __syncthreads();
                }
            }
            // var = z . z, mean = z . c + beta: lane g over the components g, g + 16, .., then the butterfly
            float sv = 0.f, sm = 0.f;
            for (int i = g; i < f; i += 16) {
                const float z = x[i];
                sv = fmaf(z, z, sv);
                if (!empty) sm = fmaf(z, cv[i], sm);
            }
            sv = ex_sum16(sv);
            sm = ex_sum16(sm);
            if (g == 0 && grp < cnt) {
                const bool live = s_tgt[grp] >= 0;
                if (out_var) out_var[u * T + t0 + grp] = live ? sv : 0.f;
                if (out_mean) out_mean[u * T + t0 + grp] = live ? sm + s_beta[grp] : 0.f;
            }
            __syncthreads();                                       // the next pass rewrites the slots and s_tgt
        }
        __syncthreads();                                           // the next row of this workgroup rewrites the triangle
    }
}

// ---- the noise of arbitrary triples -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void posterior_noise_kernel(uint64_t seed, const uint64_t* __restrict__ row_stream,
                                                              const int32_t* __restrict__ draws, const int32_t* __restrict__ components,
                                                              int64_t n, float* __restrict__ out_xi, uint32_t* __restrict__ out_k1k2) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t h = wmf_noise_normal_h(wmf_noise_row(seed, row_stream ? row_stream[i] : (uint64_t)i), draws[i], components[i]);
        if (out_k1k2) {
            out_k1k2[2 * i] = (uint32_t)(h >> 41);
            out_k1k2[2 * i + 1] = (uint32_t)(h >> 18) & 0x7FFFFFu;
        }
        if (out_xi) out_xi[i] = wmf_noise_normal(h);
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
int64_t wmf_posterior_ws_bytes(void) {
    return WMF_POSTERIOR_WS_BYTES;                                 // every width fits LDS: the workspace is reserved, never touched
}

int wmf_launch_posterior_draw(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                              const float* values, int64_t n, int n_draws, float sigma, uint64_t seed, const uint64_t* row_stream,
                              float* X_out, int32_t* fail_count, hipStream_t st) {
    const int64_t grid = n < WMF_POSTERIOR_MAX_BLOCKS ? n : WMF_POSTERIOR_MAX_BLOCKS;
    const size_t lds = po_draw_lds_bytes(f);
    WMF_LAUNCH_LDS("posterior_draw_kernel", posterior_draw_kernel, po_draw_lds_bytes(WMF_MAX_F), dim3((unsigned)grid), dim3(256), lds, st, Y, f,
                   ld, bias, W, indptr, indices, values, n, n_draws, sigma, seed, row_stream, X_out, fail_count);
    return WMF_L_OK;
}

int wmf_launch_posterior_score(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                               const float* values, int64_t n, const int32_t* targets, int n_targets, float* out_mean, float* out_var,
                               int32_t* fail_count, hipStream_t st) {
    const int64_t grid = n < WMF_POSTERIOR_MAX_BLOCKS ? n : WMF_POSTERIOR_MAX_BLOCKS;
    const size_t lds = po_score_lds_bytes(f);
    WMF_LAUNCH_LDS("posterior_score_kernel", posterior_score_kernel, po_score_lds_bytes(WMF_MAX_F), dim3((unsigned)grid), dim3(256), lds, st, Y,
                   f, ld, bias, W, indptr, indices, values, n, targets, n_targets, out_mean, out_var, fail_count);
    return WMF_L_OK;
}

void wmf_launch_posterior_noise(uint64_t seed, const uint64_t* row_stream, const int32_t* draws, const int32_t* components, int64_t n,
                                float* out_xi, uint32_t* out_k1k2, hipStream_t st) {
    int64_t grid = (n + 255) / 256;
    if (grid > WMF_POSTERIOR_NOISE_GRID) grid = WMF_POSTERIOR_NOISE_GRID;
    WMF_LAUNCH("posterior_noise_kernel", posterior_noise_kernel, dim3((unsigned)grid), dim3(256), 0, st, seed, row_stream, draws, components, n,
               out_xi, out_k1k2);
}
