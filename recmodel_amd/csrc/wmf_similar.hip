// Neighbours in factor space (gfx950): the topn rows of a catalogue matrix closest to each query row, by dot product or cosine
// over the feature columns [bias, f) -- "which items are like this one", and the same for users.
//
//   * row_inv_norms_kernel -- 1 / |row| over the feature columns, one pass: the squares are exact in float64 and are summed there
//                             in a fixed order (16 lanes a row, each its pieces in turn, then a butterfly), so two runs agree to
//                             the bit; 0 for a zero row and for an inverse that float32 cannot hold.
//   * similar_scan_kernel  -- the catalogue scan of wmf_scan.h with the top-n epilogue of wmf_topn.h and a second scoring rule:
//                             column 0 of a bias model is left out of both operands and nothing is added; the sum is then
//                             multiplied by the query's scale and by the catalogue row's, two float32 multiplications in that
//                             order.  The scales are applied AFTER the sum, so the MFMA chain is the score tile's own and the dot
//                             product is bit for bit what wmf_recommend_topn computes on the same columns; scaled operands would
//                             round every product differently and cost a pass over the catalogue.  The query's scale sits in
//                             registers next to the row's pieces.  The catalogue row's scale travels with the stage: the first
//                             16 TPS threads request it with the stage's global loads and store it to LDS with the stage's rows,
//                             so the epilogue reads it from LDS -- no global load between the MFMAs and the key.  Without scales
//                             both are 1.0f, which changes no bit.  The row's own id is refused where the exclusion list is
//                             looked up, at insertion: nothing of it is in the scoring loop.
// The partial lists are merged by recommend_merge_kernel; the result cannot depend on the slices (distinct keys, wmf_recommend.hip).

#include "wmf_common.h"
#include "wmf_internal.h"
#include "wmf_scan.h"
#include "wmf_topn.h"

#define WMF_NORMS_GRID 1024          /* workgroups of row_inv_norms_kernel: rows beyond 16 x this take another trip */
#define WMF_NORMS_ROWS 16            /* rows of a workgroup: 16 lanes a row, four rows a wave */

__global__ __launch_bounds__(256) void row_inv_norms_kernel(const float* __restrict__ M, int64_t n, int f, int ld, int bias,
                                                            float* __restrict__ out) {
    const int sub = threadIdx.x & 15, nch = ld >> 2;
    const float4* M4 = reinterpret_cast<const float4*>(M);
    for (int64_t i0 = (int64_t)blockIdx.x * WMF_NORMS_ROWS; i0 < n; i0 += (int64_t)gridDim.x * WMF_NORMS_ROWS) {
        const int64_t i = i0 + (threadIdx.x >> 4);
        double s = 0.0;
        if (i < n) {
            for (int c = sub; c < nch; c += 16) {                  // columns 4 c .. 4 c + 3; padding and the bias column are no features
                const float4 v = M4[i * nch + c];
                const double x = v.x, y = v.y, z = v.z, w = v.w;
                const int col = 4 * c;
                if (col >= bias && col < f) s += x * x;
                if (col + 1 < f) s += y * y;
                if (col + 2 < f) s += z * z;
                if (col + 3 < f) s += w * w;
            }
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);     // (a + b = b + a: the 16 lanes of a row end with the same bits)
        if (sub == 0 && i < n) {
            float r = 0.f;
            if (s > 0.0) {
                const float v = (float)(1.0 / sqrt(s));
                if (v < __builtin_inff()) r = v;
            }
            out[i] = r;
        }
    }
}

// The scan's second scoring rule: (sum over the feature columns * the query's scale) * the catalogue row's scale.
// LDS: two stages of TPS x 16 catalogue scales.
template <int TPS>
struct WmfScaledScore {
    const float* __restrict__ q_scale; const float* __restrict__ c_scale;
    float* cs;
    static constexpr bool SCALED = true;
    float pre;                                                     // this thread's scale of the stage on its way (threads < 16 TPS)

    __device__ __forceinline__ void rows(float (&rs)[4], const int32_t* __restrict__ query_idx, int64_t u0, int64_t n_rows, int q) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) rs[reg] = q_scale ? q_scale[query_idx[min(u0 + 4 * q + reg, n_rows - 1)]] : 1.f;
    }
    __device__ __forceinline__ void load(int64_t tile_first, int64_t n_items) {
        if (threadIdx.x < TPS * 16) pre = c_scale ? c_scale[min(16 * tile_first + (int64_t)threadIdx.x, n_items - 1)] : 1.f;
    }
    __device__ __forceinline__ void store(int buf) {
        if (threadIdx.x < TPS * 16) cs[buf * TPS * 16 + threadIdx.x] = pre;
    }
    __device__ __forceinline__ float item(int r, int buf, int j) { return cs[buf * TPS * 16 + 16 * j + r]; }
    __device__ __forceinline__ float score(float acc, float rs, float is) { return (acc * rs) * is; }
};

// NIT, TPS, NW: as recommend_scan_kernel.  The row's own id (self_idx) is always tested; MASK: an allow mask per query as well
// (wmf_filter.h), and the row's own id is still refused when the mask allows it.  There is no list form.
template <int NIT, int TPS, int NW, bool MASK>
__global__ __launch_bounds__(64 * NW) void similar_scan_kernel(const float* __restrict__ queries, const float* __restrict__ catalogue, int ld,
                                                               int bias, const float* __restrict__ q_scale, const float* __restrict__ c_scale,
                                                               const int32_t* __restrict__ query_idx, int64_t n_queries, int64_t n_rows,
                                                               WMF_FILTER_PARAMS, int topn, int cap, int n_slices,
                                                               int64_t tiles_per_slice, int64_t n_work, unsigned long long* __restrict__ partial) {
    extern __shared__ __align__(16) unsigned char wmf_scan_smem[];
    static_assert(TPS * 16 <= 64 * NW, "one thread per catalogue scale of a stage");
    RecTopN<NW, true, MASK> p{WMF_FILTER_FROM_PARAMS, n_queries, topn, cap, n_slices, partial};
    WmfScaledScore<TPS> sp{q_scale, c_scale, reinterpret_cast<float*>(wmf_scan_smem + wmf_scan_stage_bytes(TPS, ld) + rec_lds_bytes(NW, cap))};
    wmf_catalogue_scan<NIT, TPS, NW>(queries, catalogue, ld, bias, query_idx, n_queries, n_rows, n_slices, tiles_per_slice, n_work, p, sp);
}

// ---- launchers --------------------------------------------------------------------------------------------------------------
void wmf_launch_row_inv_norms(const float* M, int64_t n, int f, int ld, int bias, float* out, hipStream_t st) {
    int64_t grid = (n + WMF_NORMS_ROWS - 1) / WMF_NORMS_ROWS;
    if (grid > WMF_NORMS_GRID) grid = WMF_NORMS_GRID;
    WMF_LAUNCH("row_inv_norms_kernel", row_inv_norms_kernel, dim3((unsigned)grid), dim3(256), 0, st, M, n, f, ld, bias ? 1 : 0, out);
}

// flt: the exclusion lists as its seen lists, self_idx = query_idx to leave every row out of its own list, allow masks or none
int wmf_launch_similar(const float* queries, const float* catalogue, int ld, int bias, const float* q_inv_norm, const float* c_inv_norm,
                       const int32_t* query_idx, int64_t n_queries, int64_t n_rows, const WmfRowFilter& flt, int64_t topn, int32_t n_slices,
                       int32_t* out_rows, float* out_scores, int32_t* out_count, void* ws, hipStream_t st) {
    WmfScanArgs a = {queries, catalogue, ld, bias, query_idx, n_queries, n_rows, wmf_recommend_slices(n_queries, n_rows, topn, n_slices), st};
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(ws);
    const int n = (int)topn, cap = rec_cap(topn);
    const int rc = wmf_dispatch_scan(ld, [&](auto nit, auto tps) {
        return wmf_dispatch_list<4, 2>(rec_waves(topn), [&](auto nw) {
            return wmf_dispatch_list<0, 1>(flt.allow_bits ? 1 : 0, [&](auto form) {
                constexpr int NIT = decltype(nit)::value, TPS = decltype(tps)::value, NW = decltype(nw)::value;
                constexpr bool MASK = decltype(form)::value == 1;
                wmf_scan_geometry(a, NW);
                static const char* name = wmf_kname("similar_scan_%skernel<%d, %d, %d>", MASK ? "mask_" : "", NIT, TPS, NW);
                WMF_LAUNCH_LDS(name, (similar_scan_kernel<NIT, TPS, NW, MASK>), 112 * 1024, dim3((unsigned)a.grid), dim3(64 * NW),
                               wmf_scan_stage_bytes(TPS, ld) + rec_lds_bytes(NW, cap) + (size_t)2 * TPS * 16 * 4, st, a.users, a.items, a.ld, a.bias,
                               q_inv_norm, c_inv_norm, a.user_idx, a.n_rows, a.n_items, WMF_FILTER_ARGS(flt), n, cap, a.n_slices, a.tiles_per_slice, a.n_work,
                               partial);
                return (int)WMF_L_OK;
            });
        });
    });
    if (rc) return rc;
    wmf_launch_topn_merge(partial, n_queries, a.n_slices, n, out_rows, out_scores, out_count, st);
    return WMF_L_OK;
}
