// Fold a history in (gfx950): for every row u of a CSR the factors a user half step would give it against the fixed side Y,
//     x_u = A_u^-1 sum_e (w_e + 1) y~_j,      A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T
// over the stored entries e = (j, c_e) of the row (RecModel/wmf_model.py:213-240 / :311-351), solved in whitened coordinates
// q = y~ W_white:  (I + E_u) g = b,  E_u = sum_e w_e q_j q_j^T,  b = sum_e (w_e + 1) q_j,  x_u = W_white g.  Definitions:
// include/wmf_hip.h, wmf_foldin_rows; derivation and LDS budget: DESIGN.md section 5.
//
// One 256-thread workgroup per row, grid-stride over the rows; everything of a row lives in LDS (dynamic, sized by f):
//     tri   packed lower triangle of f + 1 rows (wmf_rowsystem.h): rows 0 .. f - 1 are I + E_u, row f is b, then L^-1 b, then g
//     raw   8 rows of f floats: the gathered chunk
//     qb    8 rows of f floats: the whitened chunk; the scaled pivot column of the factorisation (f + 1 floats)
//     dinv  1 / L[k][k]
// Phases: (1), (2) rs_factor_row<true>: the factorisation leaves L^-1 b in row f, so there is no forward substitution; (3) L^T g =
// L^-1 b in place, the whole workgroup on the one right-hand side, one barrier a pivot; (4) x = W_white g over b >= a, a 16-lane
// group per component; (5) the row of X_out and the zeros of its padding.
// No floating-point atomics, fixed orders everywhere: a row's arithmetic depends on nothing but the row.
#include "wmf_common.h"
#include "wmf_rowsystem.h"

// floats of a row's LDS: the triangle of f + 1 rows, raw and qb (8 f each), dinv.  The one budget: the launch and the kernel's
// ceiling both come from here.
static inline size_t fi_lds_bytes(int f) { return (size_t)(rs_tri_floats(f + 1) + (2 * EX_CHUNK + 1) * f) * sizeof(float); }

__global__ __launch_bounds__(256) void foldin_kernel(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                                     const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                     const float* __restrict__ vals, int64_t n, float* __restrict__ X_out,
                                                     int32_t* __restrict__ fail_count) {
    extern __shared__ float fi_lds[];
    __shared__ float s_w[EX_CHUNK];
    float* tri = fi_lds;
    float* raw = tri + rs_tri_floats(f + 1);
    float* qb = raw + EX_CHUNK * f;
    float* dinv = qb + EX_CHUNK * f;
    float* bv = tri + rs_row(f);                                   // row f of the triangle: b, then L^-1 b, then g
    const int tid = threadIdx.x;
    const float nan = __int_as_float(0x7fc00000);

    for (int64_t u = blockIdx.x; u < n; u += gridDim.x) {
        const int64_t lo = indptr[u], hi = indptr[u + 1];
        float* xo = X_out + u * ld;
        if (hi <= lo) {                                            // an empty row: zeros (wmf_model.py:274-276)
            for (int a = tid; a < ld; a += 256) xo[a] = 0.f;
            continue;                                              // (uniform; no LDS was touched)
        }
        if (rs_factor_row<true>(Y, f, ld, bias, W, indices, vals, lo, hi, tri, raw, qb, dinv, s_w)) {
            rs_backward_wg(tri, dinv, bv, f);
            __syncthreads();
            rs_unwhiten<1>(W, f, ld, bv, [&](int, int a, float v) { xo[a] = v; });
        } else {
            for (int a = tid; a < f; a += 256) xo[a] = nan;
            if (tid == 0) atomicAdd(fail_count, 1);
        }
        for (int a = f + tid; a < ld; a += 256) xo[a] = 0.f;
        __syncthreads();                                           // the next row of this workgroup rewrites the triangle and qb
    }
}

int wmf_launch_foldin(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                      const float* values, int64_t n, float* X_out, int32_t* fail_count, hipStream_t st) {
    RS_LAUNCH("foldin_kernel", foldin_kernel, fi_lds_bytes, f, n, st, Y, f, ld, bias, W, indptr, indices, values, n, X_out, fail_count);
    return WMF_L_OK;
}
