// The row system in LDS (gfx950): what the one-workgroup-per-row kernels that build and solve a row's own normal equations share
// (wmf_explain.hip, wmf_foldin.hip, wmf_posterior.hip).  In whitened coordinates q = y~ W_white the system of row u is
//     (I + E_u) g = b,      E_u = sum_e w_e q_j q_j^T,      b = sum_e (w_e + 1) q_j      over the stored entries e = (j, c_e),
// held as a packed lower triangle and factored in place, I + E_u = L L^T.  256 threads as 16 groups of 16 lanes: a group owns a
// row of the triangle (lanes over its columns), a right-hand side ("slot") or a component of a product, so every sum over lanes
// is a butterfly inside a group.  Pure functions of their arguments: fixed summation orders, no atomics.  Everything is inlined
// into its kernel, where the LDS pointers are offsets of the kernel's own array.  Derivation and LDS budget: DESIGN.md section 5.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <hip/hip_runtime.h>
#include "wmf_internal.h"                   /* WMF_MAX_F, WMF_LAUNCH_LDS */

#define EX_CHUNK 8                          /* stored entries (or target rows) gathered and whitened at a time */
#define RS_SLOTS 16                         /* right-hand sides of a pass: one 16-lane group each */
#define WMF_ROWSYS_MAX_BLOCKS 1024          /* workgroups of a launch: more rows than this take a second trip */
#define WMF_ROWSYS_WS_BYTES 256             /* every width fits LDS: the callers' workspace is reserved, never touched */

static_assert(RS_SLOTS == 2 * EX_CHUNK, "the 16 slots are gathered as two chunks, and hold the raw and the whitened chunk of a row");

// ---- the layout ---------------------------------------------------------------------------------------------------------------
// Element (i, j <= i) of the packed triangle is at rs_row(i) + j.  Rows 0 .. f - 1 are I + E_u, then L; with a right-hand side
// there is a row f without a diagonal: b, then c = L^-1 b.
__host__ __device__ constexpr int rs_row(int i) { return i * (i + 1) / 2; }
__host__ __device__ constexpr int rs_tri_floats(int rows) { return rs_row(rows); }
// the largest user: the triangle of f + 1 rows, 16 slots, 8 staged target rows and dinv (posterior_score_kernel; explain_kernel
// has a row less)
static_assert(rs_tri_floats(WMF_MAX_F + 1) + (RS_SLOTS + EX_CHUNK + 1) * WMF_MAX_F <= 160 * 1024 / 4 - 64,
              "the row system of the widest model must fit the LDS of a CU");

// The one launch of these kernels: a workgroup per row up to the cap, the dynamic LDS of width F and its ceiling from LDS_BYTES.
#define RS_LAUNCH(NAME, KERNEL, LDS_BYTES, F, N, ST, ...)                                                                          \
    WMF_LAUNCH_LDS(NAME, KERNEL, LDS_BYTES(WMF_MAX_F), dim3((unsigned)((N) < WMF_ROWSYS_MAX_BLOCKS ? (N) : WMF_ROWSYS_MAX_BLOCKS)), \
                   dim3(256), LDS_BYTES(F), ST, __VA_ARGS__)

// ---- gathering ----------------------------------------------------------------------------------------------------------------
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

// ---- phases 1 and 2 -----------------------------------------------------------------------------------------------------------
// A non-empty row: I + E_u (and, with RHS, b as row f) into `tri`, then L (and c = L^-1 b: the factorisation carries row f along,
// so there is no forward substitution for b) in their place and 1 / L[k][k] in dinv.  The row is gathered in chunks of 8 entries,
// each chunk whitened (W_white upper triangular: a <= b only); w_e q q^T and (w_e + 1) q are added entry by entry in stored order.
// The Cholesky is right-looking, one pivot column at a time.  raw, qb: 8 f floats each (qb also holds the f + RHS floats of a
// pivot column: f >= 1).  False, for every thread alike, if a pivot is not positive and finite; true ends on a barrier.
template <bool RHS>
__device__ __forceinline__ bool rs_factor_row(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                              const int32_t* __restrict__ indices, const float* __restrict__ vals, int64_t lo, int64_t hi,
                                              float* tri, float* raw, float* qb, float* dinv, float* s_w) {
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    const int rows = f + (RHS ? 1 : 0);
    float* bv = tri + rs_row(f);
    // a group owns row i of the triangle in every pass over it, a thread component a of b: the passes need no barrier between them
    for (int i = grp; i < rows; i += 16) {
        float* row = tri + rs_row(i);
        for (int j = g; j <= i; j += 16) row[j] = (j == i && (!RHS || i < f)) ? 1.f : 0.f;
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
            float* row = tri + rs_row(i);
            for (int j = g; j <= i; j += 16) {
                float s = row[j];
#pragma unroll
                for (int e = 0; e < EX_CHUNK; ++e) s = fmaf(wq[e], qb[e * f + j], s);
                row[j] = s;
            }
        }
        if constexpr (RHS) {
            for (int a = tid; a < f; a += 256) {
                float s = bv[a];
                for (int e = 0; e < cnt; ++e) s = fmaf(s_w[e] + 1.f, qb[e * f + a], s);
                bv[a] = s;
            }
        }
        __syncthreads();                                           // the next chunk overwrites raw, qb and s_w
    }
    // the pivot is the same LDS word for every thread, so the exit is uniform (a break and one return: with a return from inside the
    // loop hipcc's code for foldin_kernel measured 3 % slower, profiles/r27_rowsystem.json)
    bool ok = true;
    float* col = qb;
    for (int k = 0; k < f; ++k) {
        const float p = tri[rs_row(k) + k];
        if (!(p > 0.f) || p > FLT_MAX) { ok = false; break; }
        const float r = 1.f / sqrtf(p);
        for (int i = k + 1 + tid; i < rows; i += 256) {
            float* e = tri + rs_row(i) + k;
            const float v = *e * r;
            *e = v;
            col[i] = v;
        }
        if (tid == 0) dinv[k] = r;
        __syncthreads();
        for (int i = k + 1 + grp; i < rows; i += 16) {
            const float ci = -col[i];
            float* row = tri + rs_row(i);
            const int last = (!RHS || i < f) ? i : f - 1;          // (row f has no diagonal)
            for (int j = k + 1 + g; j <= last; j += 16) row[j] = fmaf(ci, col[j], row[j]);
        }
        __syncthreads();
    }
    return ok;
}

// ---- 16 right-hand sides at a time ----------------------------------------------------------------------------------------------
// q_i of 16 target slots into `slot` (16 f floats), half a pass at a time through `stage` (8 f floats): tgt[s] is the item of slot s
// or -1 (an empty slot: zeros); a half from `cnt` on is not gathered at all.  Ends on a barrier.
__device__ __forceinline__ void rs_whiten_targets16(const float* __restrict__ Y, int f, int ld, int bias, const float* __restrict__ W,
                                                    const int* tgt, float* stage, float* slot, int cnt) {
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4;
    for (int h = 0; h < RS_SLOTS / EX_CHUNK; ++h) {
        if (h * EX_CHUNK >= cnt) {
            for (int x = tid; x < EX_CHUNK * f; x += 256) slot[h * EX_CHUNK * f + x] = 0.f;
            continue;                                              // (uniform)
        }
        if (grp < EX_CHUNK) {
            const int t = tgt[h * EX_CHUNK + grp];
            ex_load_row(t >= 0 ? Y + (int64_t)t * ld : nullptr, stage + grp * f, f, bias, g);
        }
        __syncthreads();
        ex_whiten8(stage, slot + h * EX_CHUNK * f, W, f, ld, EX_CHUNK);
        __syncthreads();
    }
    __syncthreads();
}

// The two substitutions below work on x = slot + grp * f, slot `grp` on the 16 lanes of group `grp`.  Only those 16 lanes ever
// touch the slot, and they are lanes of one wave; the workgroup's barrier of a step orders the step's reads of x before the one
// write that replaces what was read (forward: x[i] after the dot product over x[0 .. i); backward: x[k] after every lane has read
// it and updated its part of x[0 .. k)), and that write before the next step's reads.

// L z = q in place.  Ends on a barrier.
__device__ __forceinline__ void rs_forward16(const float* tri, const float* dinv, float* x, int f) {
    const int g = threadIdx.x & 15;
    for (int i = 0; i < f; ++i) {
        const float* row = tri + rs_row(i);
        float s = 0.f;
        for (int k = g; k < i; k += 16) s = fmaf(row[k], x[k], s);
        s = ex_sum16(s);
        if (g == 0) x[i] = (x[i] - s) * dinv[i];
        __syncthreads();
    }
}

// L^T g = x in place.  Step k: g_k = x_k / L_kk, then x_i -= L_ki g_k for i < k -- x_k is final once the steps above k are done.
// The last write (x[0]) comes after the last barrier: the caller's barrier stands before anyone else reads the slot.
__device__ __forceinline__ void rs_backward16(const float* tri, const float* dinv, float* x, int f) {
    const int g = threadIdx.x & 15;
    for (int k = f - 1; k >= 0; --k) {
        const float zk = x[k] * dinv[k];
        const float* row = tri + rs_row(k);
        for (int i = g; i < k; i += 16) x[i] = fmaf(-row[i], zk, x[i]);
        __syncthreads();                                           // every lane has read x[k] and written its part of x[0 .. k)
        if (g == 0) x[k] = zk;
    }
}

// The same for a single right-hand side x0 with the whole workgroup on it: every element sees the operations of rs_backward16 in
// the same order, so the bits are the same.  The caller's barrier follows, as above.
__device__ __forceinline__ void rs_backward_wg(const float* tri, const float* dinv, float* x0, int f) {
    const int tid = threadIdx.x;
    for (int k = f - 1; k >= 0; --k) {
        const float zk = x0[k] * dinv[k];
        const float* row = tri + rs_row(k);
        for (int i = tid; i < k; i += 256) x0[i] = fmaf(-row[i], zk, x0[i]);
        __syncthreads();                                           // every thread has read x0[k] and written its part of x0[0 .. k)
        if (tid == 0) x0[k] = zk;                                  // (read again only by the product that follows)
    }
}

// x~ = W g over b >= a for the SLOTS vectors g at slot[s * f], a group per component a and all SLOTS on every lane; lane s of the
// group hands component a of slot s to store(s, a, v).  The order of a slot's sum does not depend on SLOTS.
template <int SLOTS, typename Store>
__device__ __forceinline__ void rs_unwhiten(const float* __restrict__ W, int f, int ld, const float* slot, Store store) {
    const int g = threadIdx.x & 15, grp = threadIdx.x >> 4;
    for (int a = grp; a < f; a += 16) {
        float acc[SLOTS];
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) acc[s] = 0.f;
        for (int b = a + g; b < f; b += 16) {
            const float wv = W[(int64_t)a * ld + b];
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) acc[s] = fmaf(wv, slot[s * f + b], acc[s]);
        }
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
            const float v = ex_sum16(acc[s]);
            if (g == s) store(s, a, v);
        }
    }
}
