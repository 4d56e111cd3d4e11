// Fold a history in (gfx950): for every row u of a CSR the factors a user half step would give it against the fixed side Y,
//     x_u = A_u^-1 sum_e (w_e + 1) y~_j,      A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T
// over the stored entries e = (j, c_e) of the row (RecModel/wmf_model.py:213-240 / :311-351), solved in whitened coordinates
// q = y~ W_white:  (I + E_u) g = b,  E_u = sum_e w_e q_j q_j^T,  b = sum_e (w_e + 1) q_j,  x_u = W_white g.  Definitions:
// include/wmf_hip.h, wmf_foldin_rows; derivation and LDS budget: DESIGN.md section 5.
//
// One 256-thread workgroup per row, grid-stride over the rows; everything of a row lives in LDS (dynamic, sized by f):
//     tri   packed lower triangle of f + 1 rows, element (i, j <= i) at i (i + 1) / 2 + j: rows 0 .. f - 1 are I + E_u, row f is b
//     raw   8 rows of f floats: the gathered chunk
//     qb    8 rows of f floats: the whitened chunk; the scaled pivot column of the factorisation (f + 1 floats); then g
//     dinv  1 / L[k][k]
// Phases: (1) gather the row in chunks of 8 entries, whiten each chunk (W_white upper triangular: a <= b only), add w_e q q^T to
// the triangle and (w_e + 1) q to b, entry by entry in stored order; (2) Cholesky, right-looking, with b carried as row f: the
// factorisation leaves L^-1 b there, so there is no forward substitution; (3) L^T g = L^-1 b, one barrier a pivot; (4) x = W_white g
// over b >= a, a 16-lane group per component; (5) the row of X_out and the zeros of its padding.
// No floating-point atomics, fixed orders everywhere: a row's arithmetic depends on nothing but the row.
#include <float.h>
#include <math.h>
#include "wmf_common.h"
#include "wmf_internal.h"
#include "wmf_rowgather.h"

#define WMF_FOLDIN_MAX_BLOCKS 1024
#define WMF_FOLDIN_WS_BYTES 256

// floats of a row's LDS: the triangle of f + 1 rows, raw and qb (8 f each; qb holds the f + 1 floats of a pivot column: f >= 1), dinv.
// The one budget: the launch and the kernel's ceiling both come from here.
__host__ __device__ static inline int fi_tri_floats(int f) { return (f + 1) * (f + 2) / 2; }
static inline size_t fi_lds_bytes(int f) { return (size_t)(fi_tri_floats(f) + (2 * EX_CHUNK + 1) * f) * sizeof(float); }
static_assert((260 + 1) * (260 + 2) / 2 + 17 * 260 <= 160 * 1024 / 4 - 64, "the row system of the widest model must fit the LDS of a CU");

__global__ __launch_bounds__(256) void foldin_kernel(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                                     const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                     const float* __restrict__ vals, int64_t n, float* __restrict__ X_out,
                                                     int32_t* __restrict__ fail_count) {
    extern __shared__ float fi_lds[];
    __shared__ float s_w[EX_CHUNK];
    float* tri = fi_lds;
    float* raw = tri + fi_tri_floats(f);
    float* qb = raw + EX_CHUNK * f;
    float* dinv = qb + EX_CHUNK * f;
    float* bv = tri + f * (f + 1) / 2;                             // row f of the triangle: b, then L^-1 b
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    const float nan = __int_as_float(0x7fc00000);

    for (int64_t u = blockIdx.x; u < n; u += gridDim.x) {
        const int64_t lo = indptr[u], hi = indptr[u + 1];
        float* xo = X_out + u * ld;
        if (hi <= lo) {                                            // an empty row: zeros (wmf_model.py:274-276)
            for (int a = tid; a < ld; a += 256) xo[a] = 0.f;
            continue;                                              // (uniform; no LDS was touched)
        }

        // ---- (1) I + E_u and b: a group owns row i of the triangle in every pass, a thread component a of b
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
            __syncthreads();                                       // (also: the zeroed triangle, before the first chunk adds to it)
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
            __syncthreads();                                       // the next chunk overwrites raw, qb and s_w
        }

        // ---- (2) Cholesky of the f + 1 rows, right-looking: the pivot is the same LDS word for every thread, so the exit is uniform
        bool ok = true;
        float* col = qb;
        for (int k = 0; k < f; ++k) {
            const float p = tri[k * (k + 1) / 2 + k];
            if (!(p > 0.f) || p > FLT_MAX) { ok = false; break; }
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
                const int last = i < f ? i : f - 1;                // (row f has no diagonal)
                for (int j = k + 1 + g; j <= last; j += 16) row[j] = fmaf(ci, col[j], row[j]);
            }
            __syncthreads();
        }

        if (ok) {
            // ---- (3) L^T g = L^-1 b: bv[k] is final once the pivots above k are done; g goes to qb (the pivot column is done with)
            float* gv = qb;
            for (int k = f - 1; k >= 0; --k) {
                const float zk = bv[k] * dinv[k];
                const float* row = tri + k * (k + 1) / 2;
                for (int i = tid; i < k; i += 256) bv[i] = fmaf(-row[i], zk, bv[i]);
                if (tid == 0) gv[k] = zk;
                __syncthreads();
            }
            // ---- (4), (5) x = W g over b >= a, a group per component a
            for (int a = grp; a < f; a += 16) {
                float acc = 0.f;
                for (int b = a + g; b < f; b += 16) acc = fmaf(W[(int64_t)a * ld + b], gv[b], acc);
                acc = ex_sum16(acc);
                if (g == 0) xo[a] = acc;
            }
        } else {
            for (int a = tid; a < f; a += 256) xo[a] = nan;
            if (tid == 0) atomicAdd(fail_count, 1);
        }
        for (int a = f + tid; a < ld; a += 256) xo[a] = 0.f;
        __syncthreads();                                           // the next row of this workgroup rewrites the triangle and qb
    }
}

int64_t wmf_foldin_ws_bytes(int64_t n, int f) {
    (void)n; (void)f;
    return WMF_FOLDIN_WS_BYTES;                                    // every width fits LDS: the workspace is reserved, never touched
}

int wmf_launch_foldin(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                      const float* values, int64_t n, float* X_out, int32_t* fail_count, hipStream_t st) {
    const int64_t grid = n < WMF_FOLDIN_MAX_BLOCKS ? n : WMF_FOLDIN_MAX_BLOCKS;
    const size_t lds = fi_lds_bytes(f);
    WMF_LAUNCH_LDS("foldin_kernel", foldin_kernel, fi_lds_bytes(WMF_MAX_F), dim3((unsigned)grid), dim3(256), lds, st, Y, f, ld, bias, W, indptr,
                   indices, values, n, X_out, fail_count);
    return WMF_L_OK;
}
