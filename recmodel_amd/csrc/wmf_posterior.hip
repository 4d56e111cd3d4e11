// The posterior of a folded-in row (gfx950): in the probabilistic reading of the row system of wmf_foldin.hip,
//     x_u ~ N(A_u^-1 b_u, A_u^-1),      A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T,
// and in whitened coordinates q = y~ W_white, where A_u^-1 = W_white (I + E_u)^-1 W_white^T and I + E_u = L L^T,
//     a draw          x~_s      = W_white L^-T (c + sigma xi_s),       c = L^-1 b, xi_s standard normal       (posterior_draw_kernel)
//     a score's law   var(u, i) = z_i . z_i,  mean(u, i) = z_i . c + beta_i,       z_i = L^-1 q_i             (posterior_score_kernel)
// Definitions: include/wmf_hip.h, wmf_posterior_draw_rows / wmf_posterior_score_rows; derivation and LDS budget: DESIGN.md section 5.
//
// One 256-thread workgroup per row, grid-stride over the rows; everything of a row lives in LDS (dynamic, sized by f):
//     tri   packed lower triangle of f + 1 rows (wmf_rowsystem.h): rows 0 .. f - 1 are I + E_u, then L; row f is b, then c
//     slot  16 vectors of f floats: raw and qb of rs_factor_row, then the 16 right-hand sides of a pass
//     stage 8 rows of f floats, the score kernel only: the raw target rows of half a pass
//     dinv  1 / L[k][k]
// Phases 1 and 2 are rs_factor_row<true>, the fold-in's.  Then, 16 at a time with a 16-lane group per right-hand side: the draw
// kernel solves L^T g = c + sigma xi_s without touching c and multiplies by W_white; the score kernel gathers and whitens 16
// targets, solves L z = q and takes two dot products.  A pass of one draw takes the whole workgroup for the substitution instead,
// as the fold-in does: every element sees the same operations in the same order either way, so draw s has the same bits in both,
// and at sigma == 0 they are the fold-in's.
// No floating-point atomics, fixed orders everywhere: a row's arithmetic depends on nothing but the row (and its stream), a slot's on
// nothing but the slot (all 16 are always computed: empty ones hold 0).
#include "wmf_common.h"
#include "wmf_noise.h"
#include "wmf_rowsystem.h"

#define WMF_POSTERIOR_NOISE_GRID 1024

// floats of a row's LDS.  The one budget of each kernel: the launch and the kernel's ceiling both come from here.
static inline size_t po_draw_lds_bytes(int f) { return (size_t)(rs_tri_floats(f + 1) + (RS_SLOTS + 1) * f) * sizeof(float); }
static inline size_t po_score_lds_bytes(int f) { return (size_t)(rs_tri_floats(f + 1) + (RS_SLOTS + EX_CHUNK + 1) * f) * sizeof(float); }

// ---- draws --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void posterior_draw_kernel(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                                             const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                             const float* __restrict__ vals, int64_t n, int n_draws, float sigma, uint64_t seed,
                                                             const uint64_t* __restrict__ row_stream, float* __restrict__ X_out,
                                                             int32_t* __restrict__ fail_count) {
    extern __shared__ float po_lds[];
    __shared__ float s_w[EX_CHUNK];
    float* tri = po_lds;
    float* slot = tri + rs_tri_floats(f + 1);                      // 16 f floats: raw (8 f) and qb (8 f) of phases 1 and 2
    float* dinv = slot + RS_SLOTS * f;
    const float* cv = tri + rs_row(f);                             // row f of the triangle: c = L^-1 b, read by every pass
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
        const bool ok = empty || rs_factor_row<true>(Y, f, ld, bias, W, indices, vals, lo, hi, tri, slot, slot + EX_CHUNK * f, dinv, s_w);
        if (!ok) {
            for (int64_t x = tid; x < (int64_t)n_draws * ld; x += 256) xo[x] = (int)(x % ld) < f ? nan : 0.f;
            if (tid == 0) atomicAdd(fail_count, 1);
            __syncthreads();                                       // the next row of this workgroup rewrites the triangle
            continue;
        }
        const uint64_t a_row = wmf_noise_row(seed, row_stream ? row_stream[u] : (uint64_t)u);
        for (int s0 = 0; s0 < n_draws; s0 += RS_SLOTS) {
            const int cnt = n_draws - s0 < RS_SLOTS ? n_draws - s0 : RS_SLOTS;
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
            // L^T g = x in place (an empty row: L = I, g = x); one draw: the whole workgroup on slot 0, as wmf_foldin.hip
            if (!empty) {
                if (cnt == 1) rs_backward_wg(tri, dinv, slot, f);
                else rs_backward16(tri, dinv, x, f);
            }
            __syncthreads();
            // x~ = W g over b >= a, all 16 slots in every pass: the text of rs_unwhiten<16>, operation for operation, written out.  Through
            // the function this kernel was 2 % slower at 100 entries a row (profiles/r27_rowsystem.json: hipcc then keeps the 16 slot
            // pointers live through the kernel, which already spills scalar registers)
            for (int a = grp; a < f; a += 16) {
                float acc[RS_SLOTS];
#pragma unroll
                for (int s = 0; s < RS_SLOTS; ++s) acc[s] = 0.f;
                for (int b = a + g; b < f; b += 16) {
                    const float wv = W[(int64_t)a * ld + b];
#pragma unroll
                    for (int s = 0; s < RS_SLOTS; ++s) acc[s] = fmaf(wv, slot[s * f + b], acc[s]);
                }
#pragma unroll
                for (int s = 0; s < RS_SLOTS; ++s) {
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
    __shared__ float s_w[EX_CHUNK], s_beta[RS_SLOTS];
    __shared__ int s_tgt[RS_SLOTS];
    float* tri = po_lds;
    float* slot = tri + rs_tri_floats(f + 1);
    float* stage = slot + RS_SLOTS * f;
    float* dinv = stage + EX_CHUNK * f;
    const float* cv = tri + rs_row(f);
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    const float nan = __int_as_float(0x7fc00000);

    for (int64_t u = blockIdx.x; u < n; u += gridDim.x) {
        const int64_t lo = indptr[u], hi = indptr[u + 1];
        const bool empty = hi <= lo;                               // I + E_u = I and c = 0: z = q, var = |q|^2, mean = beta
        const bool ok = empty || rs_factor_row<true>(Y, f, ld, bias, W, indices, vals, lo, hi, tri, slot, slot + EX_CHUNK * f, dinv, s_w);
        if (!ok && tid == 0) atomicAdd(fail_count, 1);
        for (int t0 = 0; t0 < T; t0 += RS_SLOTS) {
            const int cnt = T - t0 < RS_SLOTS ? T - t0 : RS_SLOTS;
            if (tid < RS_SLOTS) {
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
            // q_i of the 16 slots (an empty slot: zeros), then L z = q in place
            rs_whiten_targets16(Y, f, ld, bias, W, s_tgt, stage, slot, cnt);
            float* x = slot + grp * f;
            if (!empty) rs_forward16(tri, dinv, x, f);
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
int wmf_launch_posterior_draw(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                              const float* values, int64_t n, int n_draws, float sigma, uint64_t seed, const uint64_t* row_stream,
                              float* X_out, int32_t* fail_count, hipStream_t st) {
    RS_LAUNCH("posterior_draw_kernel", posterior_draw_kernel, po_draw_lds_bytes, f, n, st, Y, f, ld, bias, W, indptr, indices, values, n, n_draws,
              sigma, seed, row_stream, X_out, fail_count);
    return WMF_L_OK;
}

int wmf_launch_posterior_score(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                               const float* values, int64_t n, const int32_t* targets, int n_targets, float* out_mean, float* out_var,
                               int32_t* fail_count, hipStream_t st) {
    RS_LAUNCH("posterior_score_kernel", posterior_score_kernel, po_score_lds_bytes, f, n, st, Y, f, ld, bias, W, indptr, indices, values, n, targets,
              n_targets, out_mean, out_var, fail_count);
    return WMF_L_OK;
}

void wmf_launch_posterior_noise(uint64_t seed, const uint64_t* row_stream, const int32_t* draws, const int32_t* components, int64_t n,
                                float* out_xi, uint32_t* out_k1k2, hipStream_t st) {
    int64_t grid = (n + 255) / 256;
    if (grid > WMF_POSTERIOR_NOISE_GRID) grid = WMF_POSTERIOR_NOISE_GRID;
    WMF_LAUNCH("posterior_noise_kernel", posterior_noise_kernel, dim3((unsigned)grid), dim3(256), 0, st, seed, row_stream, draws, components, n,
               out_xi, out_k1k2);
}
