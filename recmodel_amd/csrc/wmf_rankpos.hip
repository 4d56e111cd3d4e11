// Exact full-catalogue ranks of held-out items (gfx950): for every target item of every row of a batch, the place it takes in
// wmf_recommend_topn's order of the row -- the number of unseen items of [0, n_items) whose key is strictly above the target's.
// The dual of wmf_recommend.hip: no selection, no key buffers, no merge of lists; the same catalogue scan (wmf_scan.h) with a
// counting epilogue.
//
//   * rankpos_target_kernel -- one wave per row: the scores of the row's first WMF_RANKPOS_MAX_TARGETS targets as the diagonal
//                              use of the score tile (wmf_diag_score): the 16 A rows are 16 copies of the row's user, the B rows
//                              its targets, so the scores are bit-identical to the scan's.  The 64-bit keys (wmf_item_key: the
//                              order of wmf_recommend_topn) are sorted ascending into the workspace; targets past the limit get
//                              WMF_RANKPOS_BEYOND.
//   * rankpos_scan_kernel   -- the catalogue scan, four waves.  A key at or below the user's lowest target key beats nothing (the
//                              early-out); one above the highest beats every target (a register counter); one in between is
//                              placed among the sorted target keys in LDS and counted in the bucket "beats exactly m targets" (an
//                              LDS integer atomic).  Seen items are NOT looked up here: every item of the catalogue is counted.
//                              A unit ends with the suffix sums of its buckets added to the row's counters in the workspace by
//                              integer atomics.
//   * rankpos_finish_kernel -- one wave per row: the row's seen items scored by the same diagonal tile, one taken from every
//                              target whose key is below the seen item's; a target whose key EQUALS a seen item's is that
//                              item (same user, same item, same score) and gets WMF_RANKPOS_SEEN.  O(nnz_seen x targets).
// All accumulation is in integers, so the result cannot depend on the slices, the grid or the order of the atomics.

#include "wmf_common.h"
#include "wmf_internal.h"
#include "wmf_scan.h"

#define WMF_RANKPOS_ROW_GRID 1024    /* workgroups of the two per-row kernels, four rows each */
#define RP_T WMF_RANKPOS_MAX_TARGETS
static_assert(RP_T == 16, "the per-row kernels hold a row's targets in the 16 rows of one MFMA tile");

// Workspace of n_rows rows: [tkey: RP_T keys a row, ascending, ~0 = no target][counts: RP_T a row, by sorted slot]
// [tpos: the sorted slot of the row's p-th target][tn: targets of the row, at most RP_T]
struct RankposWs { unsigned long long* tkey; unsigned int* counts; int32_t* tpos; int32_t* tn; };
static inline RankposWs rp_carve(void* ws, int64_t n_rows) {
    char* base = static_cast<char*>(ws);
    RankposWs w;
    w.tkey = reinterpret_cast<unsigned long long*>(base);
    w.counts = reinterpret_cast<unsigned int*>(base + (size_t)n_rows * RP_T * 8);
    w.tpos = reinterpret_cast<int32_t*>(base + (size_t)n_rows * RP_T * 12);
    w.tn = reinterpret_cast<int32_t*>(base + (size_t)n_rows * RP_T * 16);
    return w;
}

__global__ __launch_bounds__(256) void rankpos_target_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld, int bias,
                                                             const int32_t* __restrict__ user_idx, int64_t n_rows, int64_t n_items,
                                                             const int64_t* __restrict__ target_indptr, const int32_t* __restrict__ target_indices,
                                                             int32_t* __restrict__ out_rank, float* __restrict__ out_score,
                                                             unsigned long long* __restrict__ tkey, unsigned int* __restrict__ counts,
                                                             int32_t* __restrict__ tpos, int32_t* __restrict__ tn) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_rows; b += (int64_t)gridDim.x * 4) {
        const int64_t t0 = target_indptr[b], n_all = target_indptr[b + 1] - t0;
        const int nt = (int)(n_all < RP_T ? (n_all < 0 ? 0 : n_all) : RP_T);
        int64_t item = r < nt ? (int64_t)target_indices[t0 + r] : 0;
        item = item < 0 ? 0 : (item >= n_items ? n_items - 1 : item);                      // (every read in range whatever the ids)
        const float s = wmf_diag_score(reinterpret_cast<const float4*>(users + (int64_t)user_idx[b] * ld),
                                      reinterpret_cast<const float4*>(items + item * ld), nch, bias, q);
        const unsigned long long key = (lane < nt) ? wmf_item_key(s, item) : ~0ull;
        int pos = 0;                                               // the key's place among the 16 of lanes 0 .. 15, ascending
#pragma unroll
        for (int o = 0; o < RP_T; ++o) {
            const unsigned long long ko = wmf_shfl64(key, o);
            pos += (ko < key || (ko == key && o < r)) ? 1 : 0;
        }
        if (lane < RP_T) {
            tkey[b * RP_T + pos] = key;
            tpos[b * RP_T + lane] = pos;
            counts[b * RP_T + lane] = 0u;
            if (lane < nt && out_score) out_score[t0 + lane] = s;
        }
        if (lane == 0) tn[b] = nt;
        for (int64_t p = RP_T + lane; p < n_all; p += 64) out_rank[t0 + p] = WMF_RANKPOS_BEYOND;
    }
}

// The scan's epilogue: counts above the users' target keys.  LDS past the stages: [sorted target keys: 16 users x RP_T per wave]
// [buckets: 16 users x (RP_T + 1) per wave].
#define RP_NW 4                      /* waves of the scan's workgroup (no key buffers to pay for) */
struct RankposCount {
    static constexpr int HB = RP_T + 1;
    const unsigned long long* __restrict__ tkey; const int32_t* __restrict__ tn;
    int64_t n_rows;
    unsigned int* __restrict__ counts;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, q = lane >> 4;
    unsigned long long* tk; int* hist;
    int64_t u0;
    unsigned long long tmin[4], tmax[4];
    int nt[4], all[4];

    __device__ __forceinline__ void begin(unsigned char* lds, int64_t u0_, int) {
        u0 = u0_;
        tk = reinterpret_cast<unsigned long long*>(lds) + wave * 16 * RP_T;
        hist = reinterpret_cast<int*>(lds + (size_t)RP_NW * 16 * RP_T * 8) + wave * 16 * HB;
        // the sorted target keys of the wave's users (a row past the batch has none) and empty buckets
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = lane + 64 * k;
            const int64_t b = u0 + (idx >> 4);
            tk[idx] = b < n_rows ? tkey[b * RP_T + (idx & 15)] : ~0ull;
        }
        for (int idx = lane; idx < 16 * HB; idx += 64) hist[idx] = 0;
        wmf_wave_sync();
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t b = u0 + 4 * q + reg;
            all[reg] = 0;
            nt[reg] = b < n_rows ? tn[b] : 0;
            tmin[reg] = tk[(4 * q + reg) * RP_T];                 // ~0 when the row has no targets: nothing passes
            tmax[reg] = tk[(4 * q + reg) * RP_T + max(nt[reg] - 1, 0)];
        }
    }
    // A key at or below the user's lowest target key beats nothing; one above the highest beats every target; one in between is
    // placed among the sorted target keys and counted in the bucket "beats exactly m targets"
    __device__ __forceinline__ void score(int reg, int, int64_t, unsigned long long key, bool in_range) {
        if (in_range && key > tmin[reg]) {
            if (key > tmax[reg]) {
                ++all[reg];
            } else {                                               // tmin < key <= tmax: the targets strictly below it
                const unsigned long long* t = tk + (4 * q + reg) * RP_T;
                int m = 1;
                while (m < nt[reg] && t[m] < key) ++m;
                atomicAdd(&hist[(4 * q + reg) * HB + m], 1);
            }
        }
    }
    __device__ __forceinline__ void tile(int) {}
    __device__ __forceinline__ void end() {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg)
            if (all[reg]) atomicAdd(&hist[(4 * q + reg) * HB + nt[reg]], all[reg]);
        wmf_wave_sync();
        // sorted slot i is beaten by every key that beats more than i targets
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = lane + 64 * k, u = idx >> 4, i = idx & 15;
            unsigned int c = 0;
            for (int m = i + 1; m <= RP_T; ++m) c += (unsigned int)hist[u * HB + m];
            if (c && u0 + u < n_rows) atomicAdd(&counts[(u0 + u) * RP_T + i], c);
        }
        wmf_wave_sync();                                           // the buckets are read before the next pair resets them
    }
};

template <int NIT, int TPS>
__global__ __launch_bounds__(64 * RP_NW) void rankpos_scan_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld,
                                                                  int bias, const int32_t* __restrict__ user_idx, int64_t n_rows,
                                                                  int64_t n_items, const unsigned long long* __restrict__ tkey,
                                                                  const int32_t* __restrict__ tn, int n_slices, int64_t tiles_per_slice,
                                                                  int64_t n_work, unsigned int* __restrict__ counts) {
    RankposCount p{tkey, tn, n_rows, counts};
    wmf_catalogue_scan<NIT, TPS, RP_NW>(users, items, ld, bias, user_idx, n_rows, n_items, n_slices, tiles_per_slice, n_work, p);
}

__global__ __launch_bounds__(256) void rankpos_finish_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld, int bias,
                                                             const int32_t* __restrict__ user_idx, int64_t n_rows, int64_t n_items,
                                                             const int64_t* __restrict__ seen_indptr, const int32_t* __restrict__ seen_indices,
                                                             const int64_t* __restrict__ target_indptr,
                                                             const unsigned long long* __restrict__ tkey, const unsigned int* __restrict__ counts,
                                                             const int32_t* __restrict__ tpos, const int32_t* __restrict__ tn,
                                                             int32_t* __restrict__ out_rank) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_rows; b += (int64_t)gridDim.x * 4) {
        const unsigned long long mine = lane < RP_T ? tkey[b * RP_T + lane] : ~0ull;         // lane i: the row's i-th lowest target key
        unsigned int above = 0;
        bool is_seen = false;
        if (seen_indptr) {
            const float4* urow = reinterpret_cast<const float4*>(users + (int64_t)user_idx[b] * ld);
            const int64_t lo = seen_indptr[b], hi = seen_indptr[b + 1];
            for (int64_t e0 = lo; e0 < hi; e0 += 16) {
                const int64_t e = e0 + r;
                int64_t id = e < hi ? (int64_t)seen_indices[e] : -1;
                if (e < hi && e > lo && seen_indices[e - 1] == (int32_t)id) id = -1;         // a duplicate counts once (the row ascends)
                const bool valid = id >= 0 && id < n_items;
                if (!valid) id = 0;
                const float s = wmf_diag_score(urow, reinterpret_cast<const float4*>(items + id * ld), nch, bias, q);
                const unsigned long long sk = (valid && q == 0) ? wmf_item_key(s, id) : 0ull;     // 0 is below every key
#pragma unroll
                for (int o = 0; o < 16; ++o) {
                    const unsigned long long ko = wmf_shfl64(sk, o);
                    above += ko > mine ? 1u : 0u;
                    is_seen = is_seen || ko == mine;
                }
            }
        }
        const int32_t val = is_seen ? WMF_RANKPOS_SEEN : (int32_t)((lane < RP_T ? counts[b * RP_T + lane] : 0u) - above);
        const int32_t got = __shfl(val, lane < RP_T ? tpos[b * RP_T + lane] : 0);            // the p-th target's sorted slot
        if (lane < tn[b]) out_rank[target_indptr[b] + lane] = got;
    }
}

// ---- launcher ---------------------------------------------------------------------------------------------------------------
int64_t wmf_rank_positions_ws_bytes(int64_t n_rows) {
    if (n_rows < 1) return WMF_RANKPOS_WS_BASE;
    return WMF_RANKPOS_WS_BASE + WMF_RANKPOS_WS_PER_ROW * n_rows;
}
static_assert(WMF_RANKPOS_WS_PER_ROW == RP_T * 16 + 4, "tkey, counts and tpos of RP_T slots and tn, per row");

int wmf_launch_rank_positions(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_rows,
                              int64_t n_items, const int64_t* seen_indptr, const int32_t* seen_indices, const int64_t* target_indptr,
                              const int32_t* target_indices, int32_t n_slices, int32_t* out_rank, float* out_score, void* ws, hipStream_t st) {
    const RankposWs w = rp_carve(ws, n_rows);
    // (topn = 1: the slices of the four-wave block of wmf_recommend.hip's scan)
    WmfScanArgs a = {users, items, ld, bias, user_idx, n_rows, n_items, wmf_recommend_slices(n_rows, n_items, 1, n_slices), st};
    wmf_scan_geometry(a, RP_NW);
    int64_t row_grid = (n_rows + 3) / 4;
    if (row_grid > WMF_RANKPOS_ROW_GRID) row_grid = WMF_RANKPOS_ROW_GRID;
    return wmf_dispatch_scan(ld, [&](auto nit, auto tps) {           // (no kernel for the width: nothing is launched)
        constexpr int NIT = decltype(nit)::value, TPS = decltype(tps)::value;
        WMF_LAUNCH("rankpos_target_kernel", rankpos_target_kernel, dim3((unsigned)row_grid), dim3(256), 0, st, users, items, ld, bias, user_idx,
                   n_rows, n_items, target_indptr, target_indices, out_rank, out_score, w.tkey, w.counts, w.tpos, w.tn);
        static const char* name = wmf_kname("rankpos_scan_kernel<%d, %d>", NIT, TPS);
        WMF_LAUNCH_LDS(name, (rankpos_scan_kernel<NIT, TPS>), 64 * 1024, dim3((unsigned)a.grid), dim3(64 * RP_NW),
                       wmf_scan_stage_bytes(TPS, ld) + (size_t)RP_NW * 16 * RP_T * 8 + (size_t)RP_NW * 16 * (RP_T + 1) * 4, st, a.users, a.items,
                       a.ld, a.bias, a.user_idx, a.n_rows, a.n_items, w.tkey, w.tn, a.n_slices, a.tiles_per_slice, a.n_work, w.counts);
        WMF_LAUNCH("rankpos_finish_kernel", rankpos_finish_kernel, dim3((unsigned)row_grid), dim3(256), 0, st, users, items, ld, bias, user_idx,
                   n_rows, n_items, seen_indptr, seen_indices, target_indptr, w.tkey, w.counts, w.tpos, w.tn, out_rank);
        return (int)WMF_L_OK;
    });
}
