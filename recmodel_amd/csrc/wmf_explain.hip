// Contributions of a user's history to a score (gfx950): for every row u of a CSR and up to WMF_EXPLAIN_MAX_TARGETS target items i,
//     contrib(u, i, e) = (w_e + 1) y~_i^T A_u^-1 y~_j      for every stored entry e = (j, c_e) of the row,
// A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T the row's normal-equation matrix (RecModel/wmf_model.py:231-239 / :343-350), solved in
// whitened coordinates q = y~ W_white, where A_u becomes I + E_u with E_u = sum_e w_e q_j q_j^T.  Definitions: include/wmf_hip.h,
// wmf_explain_rows; derivation and LDS budget: DESIGN.md section 5.
//
// One 256-thread workgroup per row, grid-stride over the rows; everything of a row lives in LDS (dynamic, sized by f):
//     tri   packed lower triangle of I + E_u, element (i, j <= i) at i (i + 1) / 2 + j; after the solve the 16 vectors t_i
//     rhs   16 columns of f floats: the raw gathered chunk while E_u is accumulated, then q_i -> z_i of the 16 target slots
//     qb    8 rows of f floats: the whitened chunk; the scaled pivot column of the factorisation; the raw target rows
//     dinv  1 / L[k][k]
// Phases: (1) gather the row in chunks of 8 entries, whiten each chunk (q = y~ W_white, W_white upper triangular: a <= b only) and
// add w_e q q^T to the triangle; (2) Cholesky, right-looking, one pivot column at a time; (3) q_i of the targets, forward and
// backward substitution for all 16 slots at once (a 16-lane group per slot); (4) t_i = W_white z_i; (5) a second pass over the row,
// (w_e + 1) y~_j . t_i, a 16-lane group per stored entry; (6) the totals, entry by entry in stored order.
// The work is split over 16 groups of 16 lanes: a group owns a row of the triangle (lanes over its columns), a slot, or a stored
// entry, so every sum over lanes is a butterfly inside a group.  No floating-point atomics, fixed orders everywhere; a row's
// arithmetic depends on nothing but the row, a slot's on nothing but the slot (all 16 slots are always computed: empty ones hold 0).
#include <float.h>
#include <math.h>
#include "wmf_common.h"
#include "wmf_internal.h"
#include "wmf_rowgather.h"                  /* EX_CHUNK, ex_sum16, ex_whiten8, ex_load_row: shared with wmf_foldin.hip */

#define EX_SLOTS WMF_EXPLAIN_MAX_TARGETS    /* target slots of a row: one 16-lane group each */
#define WMF_EXPLAIN_MAX_BLOCKS 1024
#define WMF_EXPLAIN_WS_BYTES 256

static_assert(EX_SLOTS == 16 && EX_CHUNK == 8, "the kernel's groups are 16 lanes: 16 slots, two chunks of raw target rows");

// floats of the triangle's region: the packed triangle, and room for the 16 vectors t_i that replace it (f < 31: they are larger)
__host__ __device__ static inline int ex_tri_floats(int f) {
    const int t = f * (f + 1) / 2, r = EX_SLOTS * f;
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

        // ---- (1) I + E_u: a group owns row i of the triangle in every pass, so the passes over it need no barrier between them
        for (int i = grp; i < f; i += 16) {
            float* row = tri + i * (i + 1) / 2;
            for (int j = g; j <= i; j += 16) row[j] = j == i ? 1.f : 0.f;
        }
        for (int64_t c0 = lo; c0 < hi; c0 += EX_CHUNK) {
            const int cnt = hi - c0 < EX_CHUNK ? (int)(hi - c0) : EX_CHUNK;
            if (grp < EX_CHUNK) {
                const float* src = grp < cnt ? Y + (int64_t)indices[c0 + grp] * ld : nullptr;
                ex_load_row(src, rhs + grp * f, f, bias, g);
                if (g == 0) s_w[grp] = src ? vals[c0 + grp] - (bias ? src[0] : 0.f) : 0.f;
            }
            __syncthreads();
            ex_whiten8(rhs, qb, W, f, ld, cnt);
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
            __syncthreads();                                       // the next chunk overwrites rhs, qb and s_w
        }

        // ---- (2) Cholesky, right-looking: the pivot is the same LDS word for every thread, so the exit is uniform
        bool ok = true;
        float* col = qb;
        for (int k = 0; k < f; ++k) {
            const float p = tri[k * (k + 1) / 2 + k];
            if (!(p > 0.f) || p > FLT_MAX) { ok = false; break; }
            const float r = 1.f / sqrtf(p);
            for (int i = k + 1 + tid; i < f; i += 256) {
                float* e = tri + i * (i + 1) / 2 + k;
                const float v = *e * r;
                *e = v;
                col[i] = v;
            }
            if (tid == 0) dinv[k] = r;
            __syncthreads();
            for (int i = k + 1 + grp; i < f; i += 16) {
                const float ci = -col[i];
                float* row = tri + i * (i + 1) / 2;
                for (int j = k + 1 + g; j <= i; j += 16) row[j] = fmaf(ci, col[j], row[j]);
            }
            __syncthreads();
        }

        if (ok) {
            // ---- (3) q_i of the 16 slots (an empty slot: zeros), then L y = q, L^T z = y; slot `grp` on the 16 lanes of group `grp`
            for (int h = 0; h < EX_SLOTS / EX_CHUNK; ++h) {
                if (h * EX_CHUNK >= T) {
                    for (int x = tid; x < EX_CHUNK * f; x += 256) rhs[h * EX_CHUNK * f + x] = 0.f;
                    continue;                                      // (uniform)
                }
                if (grp < EX_CHUNK) {
                    const int t = s_tgt[h * EX_CHUNK + grp];
                    ex_load_row(t >= 0 ? Y + (int64_t)t * ld : nullptr, qb + grp * f, f, bias, g);
                }
                __syncthreads();
                ex_whiten8(qb, rhs + h * EX_CHUNK * f, W, f, ld, EX_CHUNK);
                __syncthreads();
            }
            __syncthreads();
            float* x = rhs + grp * f;
            for (int i = 0; i < f; ++i) {
                const float* row = tri + i * (i + 1) / 2;
                float s = 0.f;
                for (int k = g; k < i; k += 16) s = fmaf(row[k], x[k], s);
                s = ex_sum16(s);
                if (g == 0) x[i] = (x[i] - s) * dinv[i];
                __syncthreads();
            }
            for (int k = f - 1; k >= 0; --k) {
                const float zk = x[k] * dinv[k];
                __syncthreads();                                   // every lane has read x[k] before it is replaced
                const float* row = tri + k * (k + 1) / 2;
                for (int i = g; i < k; i += 16) x[i] = fmaf(-row[i], zk, x[i]);
                if (g == 0) x[k] = zk;
                __syncthreads();
            }
            // ---- (4) t = W z over b >= a, a group per component a, into the region of the triangle (no longer needed)
            float* tb = tri;
            for (int a = grp; a < f; a += 16) {
                float acc[EX_SLOTS];
#pragma unroll
                for (int s = 0; s < EX_SLOTS; ++s) acc[s] = 0.f;
                for (int b = a + g; b < f; b += 16) {
                    const float wv = W[(int64_t)a * ld + b];
#pragma unroll
                    for (int s = 0; s < EX_SLOTS; ++s) acc[s] = fmaf(wv, rhs[s * f + b], acc[s]);
                }
#pragma unroll
                for (int s = 0; s < EX_SLOTS; ++s) {
                    const float v = ex_sum16(acc[s]);
                    if (g == s) tb[s * f + a] = v;
                }
            }
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

int64_t wmf_explain_ws_bytes(int64_t n, int f, int32_t n_targets) {
    (void)n; (void)f; (void)n_targets;
    return WMF_EXPLAIN_WS_BYTES;                                   // every width fits LDS: the workspace is reserved, never touched
}

int wmf_launch_explain(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                       const float* values, int64_t n, const int32_t* targets, int n_targets, float* out_contrib, float* out_total,
                       int32_t* fail_count, hipStream_t st) {
    const int64_t grid = n < WMF_EXPLAIN_MAX_BLOCKS ? n : WMF_EXPLAIN_MAX_BLOCKS;
    const size_t lds = ex_lds_bytes(f);
    WMF_LAUNCH_LDS("explain_kernel", explain_kernel, ex_lds_bytes(WMF_MAX_F), dim3((unsigned)grid), dim3(256), lds, st, Y, f, ld, bias, W, indptr,
                   indices, values, n, targets, n_targets, out_contrib, out_total, fail_count);
    return WMF_L_OK;
}
