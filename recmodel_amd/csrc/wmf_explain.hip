// Contributions of a user's history to a score (gfx950): for every row u of a CSR and up to WMF_EXPLAIN_MAX_TARGETS target items i,
//     contrib(u, i, e) = (w_e + 1) y~_i^T A_u^-1 y~_j      for every stored entry e = (j, c_e) of the row,
// A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T the row's normal-equation matrix (RecModel/wmf_model.py:231-239 / :343-350), solved in
// whitened coordinates q = y~ W_white, where A_u becomes I + E_u with E_u = sum_e w_e q_j q_j^T.  Definitions: include/wmf_hip.h,
// wmf_explain_rows; derivation and LDS budget: DESIGN.md section 5.
//
// One 256-thread workgroup per row, grid-stride over the rows; everything of a row lives in LDS (dynamic, sized by f):
//     tri   packed lower triangle of f rows, no right-hand side (wmf_rowsystem.h); after the solve the 16 vectors t_i
//     rhs   16 columns of f floats: the raw gathered chunk while E_u is accumulated, then q_i -> z_i of the 16 target slots
//     qb    8 rows of f floats: the whitened chunk; the scaled pivot column of the factorisation; the raw target rows
//     dinv  1 / L[k][k]
// Phases: (1), (2) rs_factor_row<false>; (3) q_i of the targets, forward and backward substitution for all 16 slots at once (a
// 16-lane group per slot); (4) t_i = W_white z_i; (5) a second pass over the row, (w_e + 1) y~_j . t_i, a 16-lane group per stored
// entry; (6) the totals, entry by entry in stored order.
// No floating-point atomics, fixed orders everywhere; a row's arithmetic depends on nothing but the row, a slot's on nothing but
// the slot (all 16 slots are always computed: empty ones hold 0).
#include "wmf_common.h"
#include "wmf_rowsystem.h"

#define EX_SLOTS WMF_EXPLAIN_MAX_TARGETS    /* target slots of a row: one 16-lane group each */

static_assert(EX_SLOTS == RS_SLOTS, "a row's targets are one pass of the row system's 16 slots");

// floats of the triangle's region: the packed triangle, and room for the 16 vectors t_i that replace it (f < 31: they are larger)
__host__ __device__ static inline int ex_tri_floats(int f) {
    const int t = rs_tri_floats(f), r = EX_SLOTS * f;
    return t > r ? t : r;
}
static inline size_t ex_lds_bytes(int f) { return (size_t)(ex_tri_floats(f) + (EX_SLOTS + EX_CHUNK + 1) * f) * sizeof(float); }

__global__ __launch_bounds__(256) void explain_kernel(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                                      const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                      const float* __restrict__ vals, int64_t n, const int32_t* __restrict__ targets, int T,
                                                      float* out_contrib, float* __restrict__ out_total, int32_t* __restrict__ fail_count) {
    extern __shared__ float ex_lds[];
    __shared__ float s_w[EX_CHUNK], s_beta[EX_SLOTS];
    __shared__ int s_tgt[EX_SLOTS];
    float* tri = ex_lds;
    float* rhs = tri + ex_tri_floats(f);
    float* qb = rhs + EX_SLOTS * f;
    float* dinv = qb + EX_CHUNK * f;
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    const float nan = __int_as_float(0x7fc00000);

    for (int64_t u = blockIdx.x; u < n; u += gridDim.x) {
        const int64_t lo = indptr[u], hi = indptr[u + 1];
        if (tid < EX_SLOTS) {
            const int t = tid < T ? targets[u * T + tid] : -1;
            s_tgt[tid] = t;
            s_beta[tid] = (t >= 0 && bias) ? Y[(int64_t)t * ld] : 0.f;
        }
        __syncthreads();
        if (hi <= lo) {                                            // an empty row: no contributions, the total is beta_i
            if (tid < T) out_total[u * T + tid] = s_tgt[tid] >= 0 ? 0.f + s_beta[tid] : 0.f;
            __syncthreads();
            continue;
        }

        // ---- (1), (2) I + E_u, then L: the raw chunk goes through the slots, not yet in use
        const bool ok = rs_factor_row<false>(Y, f, ld, bias, W, indices, vals, lo, hi, tri, rhs, qb, dinv, s_w);
        if (ok) {
            // ---- (3) q_i of the 16 slots (the raw target rows go through qb), then L y = q, L^T z = y
            rs_whiten_targets16(Y, f, ld, bias, W, s_tgt, qb, rhs, T);
            float* x = rhs + grp * f;
            rs_forward16(tri, dinv, x, f);
            rs_backward16(tri, dinv, x, f);
            __syncthreads();
            // ---- (4) t = W z, into the region of the triangle (no longer needed)
            float* tb = tri;
            rs_unwhiten<EX_SLOTS>(W, f, ld, rhs, [&](int s, int a, float v) { tb[s * f + a] = v; });
            __syncthreads();
            // ---- (5) the second pass over the row: a group per stored entry
            for (int64_t e = lo + grp; e < hi; e += 16) {
                const float* src = Y + (int64_t)indices[e] * ld;
                float acc[EX_SLOTS];
#pragma unroll
                for (int s = 0; s < EX_SLOTS; ++s) acc[s] = 0.f;
                for (int a = g; a < f; a += 16) {
                    const float y = (bias && a == 0) ? 1.f : src[a];
#pragma unroll
                    for (int s = 0; s < EX_SLOTS; ++s) acc[s] = fmaf(y, tb[s * f + a], acc[s]);
                }
                const float wp1 = (vals[e] - (bias ? src[0] : 0.f)) + 1.f;
#pragma unroll
                for (int s = 0; s < EX_SLOTS; ++s) {
                    const float v = ex_sum16(acc[s]);
                    if (g == s && s < T) out_contrib[e * T + s] = s_tgt[s] >= 0 ? wp1 * v : 0.f;
                }
            }
        } else {
            for (int64_t x = (int64_t)tid; x < (hi - lo) * T; x += 256) out_contrib[lo * T + x] = s_tgt[x % T] >= 0 ? nan : 0.f;
            if (tid == 0) atomicAdd(fail_count, 1);
        }
        // ---- (6) totals: the row's contributions in stored order, then beta_i (what the workgroup wrote, after the barrier)
        __syncthreads();
        if (tid < T) {
            float s = 0.f;
            for (int64_t e = lo; e < hi; ++e) s += out_contrib[e * T + tid];
            s += s_beta[tid];
            out_total[u * T + tid] = s_tgt[tid] >= 0 ? (ok ? s : nan) : 0.f;
        }
        __syncthreads();                                           // the next row of this workgroup rewrites the slots
    }
}

int wmf_launch_explain(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                       const float* values, int64_t n, const int32_t* targets, int n_targets, float* out_contrib, float* out_total,
                       int32_t* fail_count, hipStream_t st) {
    RS_LAUNCH("explain_kernel", explain_kernel, ex_lds_bytes, f, n, st, Y, f, ld, bias, W, indptr, indices, values, n, targets, n_targets,
              out_contrib, out_total, fail_count);
    return WMF_L_OK;
}
