// Audit of a half step (gfx950): the implicit-feedback objective the half step minimises and, per row, what is needed for the
// normwise backward error of the row's normal equations A_u x_u = b_u (RecModel/wmf_model.py:237-239 / :343-350) -- in float64 on
// the factors as stored, in one pass over the CSR, independent of every solver path.  Definitions: include/wmf_hip.h,
// wmf_half_step_audit.
//
// One wave per CSR row, four stored entries in flight (one per 16-lane group), a lane holds the 16-byte pieces gl, gl + 16, ... of a
// factor row -- the shape of eval_kernel (wmf_eval.hip).  The per-lane accumulators are arrays indexed at compile time (templated
// on the pieces per lane, 1 .. 5 for ld <= 272): a run-time index would put them into scratch.  Rows above WMF_HEAVY_T entries
// are put on a device-side list (the way wmf_iter.hip hands rows back) and get a 256-thread workgroup each in a second launch;
// what such a row contributes to the sums is stored under its row id and folded in row order, so neither a row's result nor the
// sums depend on the order of the list.  No floating-point atomics; every reduction has a fixed order: two runs are bit-identical.
#include "wmf_common.h"
#include "wmf_internal.h"

#define WMF_AUDIT_HEAVY_BLOCKS 1024

// columns 4 c .. 4 c + 3 of a factor row as float64: one 16-byte load of a padded float32 row (padding columns are zero), four
// guarded 8-byte loads of a dense float64 row (f may be odd)
__device__ __forceinline__ void audit_load4(const float* __restrict__ row, int c, int f, double (&o)[4]) {
    (void)f;
    const float4 v = reinterpret_cast<const float4*>(row)[c];
    o[0] = (double)v.x; o[1] = (double)v.y; o[2] = (double)v.z; o[3] = (double)v.w;
}
__device__ __forceinline__ void audit_load4(const double* __restrict__ row, int c, int f, double (&o)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = 4 * c + j < f ? row[4 * c + j] : 0.0;
}

// sum over the 16 lanes of a group, the same bits on every lane (each stage adds the two partners' values, which commutes)
__device__ __forceinline__ double audit_sum16(double v) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the four groups of a wave: (g0 + g1) + (g2 + g3) on every lane
__device__ __forceinline__ double audit_sum_groups(double v) {
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

template <int P, bool ROWS>
struct AuditAcc {
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;      // (1 + w)(1 - s)^2, s^2, entries: on lane 0 of each group
    double a = 0.0;                             // |w| times this lane's share of |y~|^2
    double r[ROWS ? P : 1][4], b[ROWS ? P : 1][4];
    __device__ __forceinline__ void clear_row() {
        a = 0.0;
#pragma unroll
        for (int p = 0; p < (ROWS ? P : 1); ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j) r[p][j] = b[p][j] = 0.0;
    }
};

template <int P, class T>
__device__ __forceinline__ void audit_load_row(const T* __restrict__ row, int gl, int nch, int f, double (&x)[P][4]) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const int c = gl + 16 * p;
        if (c < nch) audit_load4(row, c, f, x[p]);
        else x[p][0] = x[p][1] = x[p][2] = x[p][3] = 0.0;
    }
}

// one stored entry (u, i, v) on the 16 lanes of a group; `act` = false: a lane group past the end of the row (it still takes part
// in the group sum)
template <int P, bool ROWS, class T>
__device__ __forceinline__ void audit_entry(const double (&x)[P][4], const T* __restrict__ yi, double v, bool act, int gl, int nch, int f,
                                            int bias, AuditAcc<P, ROWS>& acc) {
    double y[P][4];
    audit_load_row<P>(yi, gl, nch, f, y);
    double beta = 0.0;
    if (bias) {
        beta = (double)yi[0];
        if (gl == 0) y[0][0] = 1.0;
    }
    double dot = 0.0;
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) dot += x[p][j] * y[p][j];
    const double s = audit_sum16(dot);
    if (!act) return;
    const double w = v - beta;
    if (gl == 0) {
        acc.s1 += (1.0 + w) * ((1.0 - s) * (1.0 - s));
        acc.s2 += s * s;
        acc.cnt += 1.0;
    }
    if constexpr (ROWS) {
        const double coef = w * s - (w + 1.0), wp = w + 1.0;
        double nrm = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                nrm += y[p][j] * y[p][j];
                acc.r[p][j] += coef * y[p][j];
                acc.b[p][j] += wp * y[p][j];
            }
        acc.a += fabs(w) * nrm;
    }
}

// |r + dense|^2 and |b|^2 of a row whose r, b pieces are complete on (at least) the 16 lanes of the calling group
template <int P>
__device__ __forceinline__ void audit_row_norms(const double (&r)[P][4], const double (&b)[P][4], const double* __restrict__ dense_u, int gl,
                                                int f, double& rr, double& bb) {
    rr = 0.0; bb = 0.0;
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * (gl + 16 * p) + j;
            if (col < f) {
                const double t = r[p][j] + dense_u[col];
                rr += t * t;
                bb += b[p][j] * b[p][j];
            }
        }
    rr = audit_sum16(rr);
    bb = audit_sum16(bb);
}

// block partial of the three sums -> partial[blockIdx][3], the four waves in order
__device__ __forceinline__ void audit_block_sums(double s1, double s2, double cnt, double* __restrict__ partial) {
    __shared__ double red[4][3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    s1 = wmf_wave_sum_f64(s1); s2 = wmf_wave_sum_f64(s2); cnt = wmf_wave_sum_f64(cnt);
    if (lane == 0) { red[wv][0] = s1; red[wv][1] = s2; red[wv][2] = cnt; }
    __syncthreads();
    if (threadIdx.x < 3)
        partial[(int64_t)blockIdx.x * 3 + threadIdx.x] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}

// nch: 16-byte pieces (float32) or groups of four columns (float64) of a factor row; ldx: elements between two rows
template <int P, bool ROWS, class T>
__global__ __launch_bounds__(256) void audit_kernel(const T* __restrict__ X, const T* __restrict__ Y, int f, int ldx, int nch, int bias,
                                                    const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                    const T* __restrict__ vals, int64_t n, const double* __restrict__ dense,
                                                    double* __restrict__ out_rows, double* __restrict__ partial,
                                                    int32_t* __restrict__ heavy_count, int32_t* __restrict__ heavy_list) {
    const int lane = threadIdx.x & 63, gl = lane & 15, grp = lane >> 4;
    AuditAcc<P, ROWS> acc;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < n; u += (int64_t)gridDim.x * 4) {
        const int64_t lo = indptr[u], hi = indptr[u + 1];
        if (hi - lo > WMF_HEAVY_T) {                               // a workgroup of the second launch takes the row
            if (lane == 0) heavy_list[atomicAdd(heavy_count, 1)] = (int32_t)u;   // (each row at most once: the list holds n)
            continue;
        }
        double x[P][4];
        audit_load_row<P>(X + u * (int64_t)ldx, gl, nch, f, x);
        if constexpr (ROWS) acc.clear_row();
        for (int64_t jb = lo; jb < hi; jb += 4) {                  // uniform trip count across the 4 groups
            const int64_t j = jb + grp;
            const bool act = j < hi;
            const int64_t e = act ? j : lo;                        // lo < hi inside this loop: a valid entry
            audit_entry<P, ROWS>(x, Y + (int64_t)indices[e] * ldx, (double)vals[e], act, gl, nch, f, bias, acc);
        }
        if constexpr (ROWS) {
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int j = 0; j < 4; ++j) { acc.r[p][j] = audit_sum_groups(acc.r[p][j]); acc.b[p][j] = audit_sum_groups(acc.b[p][j]); }
            double rr, bb;
            audit_row_norms<P>(acc.r, acc.b, dense + u * (int64_t)f, gl, f, rr, bb);
            const double a = wmf_wave_sum_f64(acc.a);
            if (lane == 0) { out_rows[u * 3] = rr; out_rows[u * 3 + 1] = bb; out_rows[u * 3 + 2] = a; }
        }
    }
    audit_block_sums(acc.s1, acc.s2, acc.cnt, partial);
}

// the rows of the list, one 256-thread workgroup per row: 16 entries in flight; the waves' sums, r and b are combined through LDS
// in wave order.  row_sums[u][3] = what row u adds to S1, S2, N.
template <int P, bool ROWS, class T>
__global__ __launch_bounds__(256) void audit_heavy_kernel(const T* __restrict__ X, const T* __restrict__ Y, int f, int ldx, int nch, int bias,
                                                          const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                          const T* __restrict__ vals, const double* __restrict__ dense,
                                                          double* __restrict__ out_rows, double* __restrict__ row_sums,
                                                          const int32_t* __restrict__ heavy_count, const int32_t* __restrict__ heavy_list) {
    __shared__ double red_v[ROWS ? 2 : 1][4][P * 64];              // [r | b][wave][piece p, element j, lane gl]
    __shared__ double red_s[4][4];
    const int lane = threadIdx.x & 63, gl = lane & 15, grp = lane >> 4, wv = threadIdx.x >> 6;
    const int count = *heavy_count;
    for (int k = blockIdx.x; k < count; k += gridDim.x) {
        const int64_t u = heavy_list[k];
        const int64_t lo = indptr[u], hi = indptr[u + 1];
        AuditAcc<P, ROWS> acc;
        if constexpr (ROWS) acc.clear_row();
        double x[P][4];
        audit_load_row<P>(X + u * (int64_t)ldx, gl, nch, f, x);
        for (int64_t jb = lo; jb < hi; jb += 16) {                 // uniform trip count across the 16 groups
            const int64_t j = jb + wv * 4 + grp;
            const bool act = j < hi;
            const int64_t e = act ? j : lo;
            audit_entry<P, ROWS>(x, Y + (int64_t)indices[e] * ldx, (double)vals[e], act, gl, nch, f, bias, acc);
        }
        const double s1 = wmf_wave_sum_f64(acc.s1), s2 = wmf_wave_sum_f64(acc.s2), cnt = wmf_wave_sum_f64(acc.cnt);
        const double a = wmf_wave_sum_f64(acc.a);
        if (lane == 0) { red_s[wv][0] = s1; red_s[wv][1] = s2; red_s[wv][2] = cnt; red_s[wv][3] = a; }
        if constexpr (ROWS) {
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double r = audit_sum_groups(acc.r[p][j]), b = audit_sum_groups(acc.b[p][j]);
                    if (grp == 0) { red_v[0][wv][(p * 4 + j) * 16 + gl] = r; red_v[1][wv][(p * 4 + j) * 16 + gl] = b; }
                }
        }
        __syncthreads();
        if (threadIdx.x < 3) row_sums[u * 3 + threadIdx.x] = ((red_s[0][threadIdx.x] + red_s[1][threadIdx.x]) + red_s[2][threadIdx.x]) + red_s[3][threadIdx.x];
        if constexpr (ROWS) {
            if (wv == 0 && grp == 0) {
                double r[P][4], b[P][4];
#pragma unroll
                for (int p = 0; p < P; ++p)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = (p * 4 + j) * 16 + gl;
                        r[p][j] = ((red_v[0][0][i] + red_v[0][1][i]) + red_v[0][2][i]) + red_v[0][3][i];
                        b[p][j] = ((red_v[1][0][i] + red_v[1][1][i]) + red_v[1][2][i]) + red_v[1][3][i];
                    }
                double rr, bb;
                audit_row_norms<P>(r, b, dense + u * (int64_t)f, gl, f, rr, bb);
                if (gl == 0) {
                    out_rows[u * 3] = rr; out_rows[u * 3 + 1] = bb;
                    out_rows[u * 3 + 2] = ((red_s[0][3] + red_s[1][3]) + red_s[2][3]) + red_s[3][3];
                }
            }
        }
        __syncthreads();                                           // the next row of this workgroup writes the same LDS
    }
}

// what the listed rows add to the sums, taken in row order (one thread per row of a fixed grid): partial2[blockIdx][3]
__global__ __launch_bounds__(256) void audit_fold_kernel(const int64_t* __restrict__ indptr, int64_t n, const int32_t* __restrict__ heavy_count,
                                                         const double* __restrict__ row_sums, double* __restrict__ partial2) {
    double s1 = 0.0, s2 = 0.0, cnt = 0.0;
    if (*heavy_count > 0) {
        for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < n; u += (int64_t)gridDim.x * 256) {
            if (indptr[u + 1] - indptr[u] > WMF_HEAVY_T) { s1 += row_sums[u * 3]; s2 += row_sums[u * 3 + 1]; cnt += row_sums[u * 3 + 2]; }
        }
    }
    audit_block_sums(s1, s2, cnt, partial2);
}

__global__ void audit_finish_kernel(const double* __restrict__ partial, int nblocks, const double* __restrict__ partial2, int nblocks2,
                                    double* __restrict__ out3) {
    const int k = threadIdx.x;
    if (k >= 3) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += partial[(int64_t)b * 3 + k];     // fixed order: reproducible
    for (int b = 0; b < nblocks2; ++b) s += partial2[(int64_t)b * 3 + k];
    out3[k] = s;
}

// workspace: [block partials of the row pass | of the fold pass | list counter | list of n row ids | n x 3 row sums]
static inline int64_t audit_list_off() { return (int64_t)2 * WMF_AUDIT_MAX_BLOCKS * 3 * sizeof(double) + 256; }
static inline int64_t audit_sums_off(int64_t n) { return audit_list_off() + ((n * 4 + 255) & ~(int64_t)255); }
int64_t wmf_audit_ws_bytes(int64_t n) {
    if (n < 0) n = 0;
    return audit_sums_off(n) + n * 3 * (int64_t)sizeof(double);
}

template <int P, bool ROWS, class T>
static int audit_launch(const T* X, const T* Y, int f, int ldx, int nch, int bias, const int64_t* indptr, const int32_t* indices,
                        const T* values, int64_t n, const double* dense, double* out_sums, double* out_rows, void* ws, hipStream_t st) {
    char* base = (char*)ws;
    double* partial = (double*)base;
    double* partial2 = partial + (int64_t)WMF_AUDIT_MAX_BLOCKS * 3;
    int32_t* count = (int32_t*)(base + audit_list_off() - 256);
    int32_t* list = (int32_t*)(base + audit_list_off());
    double* row_sums = (double*)(base + audit_sums_off(n));
    if (hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess) return WMF_L_HIP;
    int64_t grid = (n + 3) / 4;
    if (grid > WMF_AUDIT_MAX_BLOCKS) grid = WMF_AUDIT_MAX_BLOCKS;
    if (grid < 1) grid = 1;
    int64_t heavy_grid = n < 1 ? 1 : (n > WMF_AUDIT_HEAVY_BLOCKS ? WMF_AUDIT_HEAVY_BLOCKS : n);
    int64_t fold_grid = (n + 255) / 256;
    if (fold_grid > WMF_AUDIT_MAX_BLOCKS) fold_grid = WMF_AUDIT_MAX_BLOCKS;
    if (fold_grid < 1) fold_grid = 1;
    const char* ty = sizeof(T) == 4 ? "float" : "double";
    WMF_LAUNCH(wmf_kname("audit_kernel<%d, %s, %s>", P, wmf_tf(ROWS), ty), (audit_kernel<P, ROWS, T>), dim3((unsigned)grid), dim3(256), 0, st,
               X, Y, f, ldx, nch, bias, indptr, indices, values, n, dense, out_rows, partial, count, list);
    WMF_LAUNCH(wmf_kname("audit_heavy_kernel<%d, %s, %s>", P, wmf_tf(ROWS), ty), (audit_heavy_kernel<P, ROWS, T>), dim3((unsigned)heavy_grid),
               dim3(256), 0, st, X, Y, f, ldx, nch, bias, indptr, indices, values, dense, out_rows, row_sums, count, list);
    WMF_LAUNCH("audit_fold_kernel", audit_fold_kernel, dim3((unsigned)fold_grid), dim3(256), 0, st, indptr, n, count, row_sums, partial2);
    WMF_LAUNCH("audit_finish_kernel", audit_finish_kernel, dim3(1), dim3(64), 0, st, partial, (int)grid, partial2, (int)fold_grid, out_sums);
    return WMF_L_OK;
}

template <class T>
static int audit_dispatch(const T* X, const T* Y, int f, int ldx, int nch, int bias, const int64_t* indptr, const int32_t* indices,
                          const T* values, int64_t n, const double* dense, double* out_sums, double* out_rows, void* ws, hipStream_t st) {
    return wmf_dispatch_nfb<1, 5>((nch + 15) / 16, [&](auto p) {
        constexpr int P = decltype(p)::value;
        if (out_rows) return audit_launch<P, true, T>(X, Y, f, ldx, nch, bias, indptr, indices, values, n, dense, out_sums, out_rows, ws, st);
        return audit_launch<P, false, T>(X, Y, f, ldx, nch, bias, indptr, indices, values, n, dense, out_sums, out_rows, ws, st);
    });
}

int wmf_launch_audit(const float* X, const float* Y, int f, int ld, int bias, const int64_t* indptr, const int32_t* indices,
                     const float* values, int64_t n, const double* dense, double* out_sums, double* out_rows, void* ws, hipStream_t st) {
    return audit_dispatch<float>(X, Y, f, ld, ld >> 2, bias, indptr, indices, values, n, dense, out_sums, out_rows, ws, st);
}

int wmf_launch_audit_f64(const double* X, const double* Y, int f, int bias, const int64_t* indptr, const int32_t* indices,
                         const double* values, int64_t n, const double* dense, double* out_sums, double* out_rows, void* ws, hipStream_t st) {
    return audit_dispatch<double>(X, Y, f, f, (f + 3) >> 2, bias, indptr, indices, values, n, dense, out_sums, out_rows, ws, st);
}
