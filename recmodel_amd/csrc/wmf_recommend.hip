// Full-catalogue top-N with per-user exclusions (gfx950): the N best items of [0, n_items) for every user of a batch, leaving out
// what the user has seen -- the query of RecModel/utils.py:3-17 (test_coverage ranks np.delete(arange(n_items), seen) for every
// user) through WMF.rank (RecModel/wmf_model.py:25-47), in one fused pass: nothing of size n_users x n_items exists anywhere.
//
//   * recommend_scan_kernel  -- the catalogue scan of wmf_scan.h (16 users per wave in registers, the catalogue's 16-item tiles
//                               staged in LDS slice by slice, the score tile's arithmetic: bit-identical to score_tile_kernel)
//                               with the top-n epilogue.  Every score arrives as a 64-bit key (order-preserving key of the
//                               score, ~item id): ONE total order, a higher score wins, equal scores go to the lower id.  A key
//                               that beats the user's threshold -- the current N-th best -- is looked up in the user's sorted
//                               seen list (binary search) and, if it is not there, appended to the user's LDS buffer; a buffer
//                               that could overflow on the next tile is cut back to its N best, which also raises the threshold.
//                               Insertions are rare (about N ln(n / N) per user), so neither the exclusion nor the selection
//                               costs anything in the scoring loop.
//   * recommend_merge_kernel -- the sorted partial lists of a user's slices merged by rank: a key's place is the number of
//                               keys above it, found by one binary search per slice.
//   * recommend_scan_wide_kernel, recommend_select_wide_kernel -- the same scan for 1 <= topn <= 4096 (wmf_recommend_topn_wide): the
//                               keys of a (user, slice) pair in the workspace, cut back by an exact select (wmf_topn_wide.h), and the
//                               selection and sort of the topn best of a user's slices.
//   * recommend_scan_grouped_kernel -- one list per (user, group) from one scan (wmf_recommend_topn_grouped): the wide scan with a
//                               buffer per (user, group, slice) (wmf_topn_grouped.h); recommend_select_wide_kernel finishes them.
// The keys of a user are pairwise distinct, so the result is a function of the scores alone: it cannot depend on the number of
// slices, the grid or the order in which workgroups, waves or LDS atomics finish.  No float atomics.
//
// What the three scans share exists once.  Which items may enter a list -- the row's own id, its allow mask, its seen list, tested in
// that order after the threshold -- is WmfRowFilter / WmfRowEligible (wmf_filter.h), which also says how the filter crosses a launch; the form of a
// call's filter (none, mask, list) is a template argument of each scan and the suffix of its profile name (rec_form, wmf_filter.h).  The
// in-place cut of a workspace buffer and its overwrite argument are rec_wide_cut_buffer (wmf_topn_wide.h).  A key is decoded into the
// outputs by rec_write_slot.  Each family has one launch site, its instantiation chosen by wmf_dispatch_scan x wmf_dispatch_list; the
// wide and the grouped launcher share the workspace split and the selection (rec_wide_scan_select).

#include "wmf_common.h"
#include "wmf_internal.h"
#include "wmf_scan.h"
#include "wmf_topn.h"
#include "wmf_topn_wide.h"
#include "wmf_topn_grouped.h"

#define WMF_REC_MERGE_GRID 1024      /* workgroups of the merge, four users each */
#define WMF_REC_SLICE_TILES 64       /* an automatic slice holds at least this many 16-item tiles */

// (the forms of a call's filter -- rec_form, REC_FORM_NAME, rec_form_lds -- are wmf_filter.h's)

// NIT, TPS: the scan's width class; NW: waves of a workgroup (the key buffers of 16 NW users share the LDS with the stages)
template <int NIT, int TPS, int NW, int FORM>
__global__ __launch_bounds__(64 * NW) void recommend_scan_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld,
                                                                 int bias, const int32_t* __restrict__ user_idx, int64_t n_users,
                                                                 int64_t n_items, WMF_FILTER_PARAMS, int topn, int cap, int n_slices,
                                                                 int64_t tiles_per_slice, int64_t n_work,
                                                                 unsigned long long* __restrict__ partial) {
    extern __shared__ __align__(16) unsigned char wmf_scan_smem[];
    RecTopN<NW, false, FORM == 1> p{WMF_FILTER_FROM_PARAMS, n_users, topn, cap, n_slices, partial};
    wmf_catalogue_scan<NIT, TPS, NW, decltype(p), WmfModelScore, FORM == 2>(
        users, items, ld, bias, user_idx, n_users, n_items, n_slices, tiles_per_slice, n_work, p, WmfModelScore(), cand_idx,
        reinterpret_cast<int32_t*>(wmf_scan_smem + wmf_scan_stage_bytes(TPS, ld) + rec_lds_bytes(NW, cap)));
}

// keys of `list` (topn of them, descending, 0 = none) above `key`
__device__ __forceinline__ int rec_count_above(const unsigned long long* __restrict__ list, int topn, unsigned long long key) {
    int lo = 0, hi = topn;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (list[mid] > key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wave per batch position: a key's place in the merged order is the number of keys above it over all slices
__global__ __launch_bounds__(256) void recommend_merge_kernel(const unsigned long long* __restrict__ partial, int64_t n_users, int n_slices,
                                                              int topn, int32_t* __restrict__ out_items, float* __restrict__ out_scores,
                                                              int32_t* __restrict__ out_count) {
    const int lane = threadIdx.x & 63;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_users; b += (int64_t)gridDim.x * 4) {
        const unsigned long long* P = partial + b * n_slices * topn;
        const int m = n_slices * topn;
        int mine = 0;
        for (int e = lane; e < m; e += 64) {
            const unsigned long long key = P[e];
            if (key == 0ull) continue;
            ++mine;
            int place = 0;
            for (int s = 0; s < n_slices && place < topn; ++s) place += rec_count_above(P + s * topn, topn, key);
            if (place < topn) rec_write_slot(out_items, out_scores, b * topn + place, key);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        const int count = min(mine, topn);
        for (int k = count + lane; k < topn; k += 64) rec_write_slot(out_items, out_scores, b * topn + k, 0ull);
        if (lane == 0 && out_count) out_count[b] = count;
    }
}

// ---- beyond the LDS buffers: wmf_recommend_topn_wide -----------------------------------------------------------------------------
// The same scans -- the same width classes, WmfModelScore, GATHER for the list form, so the same score bits -- with the epilogue of
// wmf_topn_wide.h: the keys of a (batch position, slice) pair in the workspace, cut back by an exact select.  Any FORM.
template <int NIT, int TPS, int NW, int FORM>
__global__ __launch_bounds__(64 * NW) void recommend_scan_wide_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld,
                                                                      int bias, const int32_t* __restrict__ user_idx, int64_t n_users,
                                                                      int64_t n_items, WMF_FILTER_PARAMS, int topn, int cap, int n_slices,
                                                                      int64_t tiles_per_slice, int64_t n_work, unsigned long long* keys_ws,
                                                                      int32_t* counts_ws) {
    extern __shared__ __align__(16) unsigned char wmf_scan_smem[];
    RecTopNWide<NW, FORM == 1> p{WMF_FILTER_FROM_PARAMS, n_users, topn, cap, n_slices, keys_ws, counts_ws};
    wmf_catalogue_scan<NIT, TPS, NW, decltype(p), WmfModelScore, FORM == 2>(
        users, items, ld, bias, user_idx, n_users, n_items, n_slices, tiles_per_slice, n_work, p, WmfModelScore(), cand_idx,
        reinterpret_cast<int32_t*>(wmf_scan_smem + wmf_scan_stage_bytes(TPS, ld) + rec_wide_lds_bytes(NW)));
}

// One workgroup per batch position: the topn best keys of all the row's slices, sorted best first in LDS (rec_wide_select_row,
// wmf_topn_wide.h), then items, scores, count and padding.
__global__ __launch_bounds__(256) void recommend_select_wide_kernel(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ counts,
                                                                    int64_t n_users, int n_slices, int topn, int cap,
                                                                    int32_t* __restrict__ out_items, float* __restrict__ out_scores,
                                                                    int32_t* __restrict__ out_count) {
    __shared__ unsigned long long sel[WMF_RECOMMEND_WIDE_MAX_TOPN];
    __shared__ unsigned hist[256];
    __shared__ int counters[2];
    const int t = threadIdx.x;
    for (int64_t b = blockIdx.x; b < n_users; b += gridDim.x) {
        const int count = rec_wide_select_row(keys + (size_t)b * n_slices * cap, counts + b * n_slices, n_slices, topn, cap, sel, hist, counters, t);
        for (int k = t; k < topn; k += 256) rec_write_slot(out_items, out_scores, b * topn + k, k < count ? sel[k] : 0ull);
        if (t == 0 && out_count) out_count[b] = count;
        __syncthreads();                                           // sel and the counters are read before the next row resets them
    }
}

// ---- one list per (row, group): wmf_recommend_topn_grouped ----------------------------------------------------------------------
// The wide scan with the epilogue of wmf_topn_grouped.h: the same width classes, waves and WmfModelScore, so the same score bits; a
// row's keys in n_groups x n_slices buffers of the workspace, laid out as recommend_select_wide_kernel reads them for n_users *
// n_groups rows.  MASK: the mask form.  There is no list form.
template <int NIT, int TPS, int NW, bool MASK>
__global__ __launch_bounds__(64 * NW) void recommend_scan_grouped_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld,
                                                                         int bias, const int32_t* __restrict__ user_idx, int64_t n_users,
                                                                         int64_t n_items, WMF_FILTER_PARAMS,
                                                                         const int32_t* __restrict__ group_of, int n_groups, int topn, int cap,
                                                                         int n_slices, int64_t tiles_per_slice, int64_t n_work,
                                                                         unsigned long long* keys_ws, int32_t* counts_ws) {
    RecTopNGrouped<TPS, NW, MASK> p{WMF_FILTER_FROM_PARAMS, n_users, topn, cap, n_slices, keys_ws, counts_ws, group_of, n_items, n_groups};
    wmf_catalogue_scan<NIT, TPS, NW>(users, items, ld, bias, user_idx, n_users, n_items, n_slices, tiles_per_slice, n_work, p);
}

// ---- launcher ---------------------------------------------------------------------------------------------------------------
int64_t wmf_recommend_ws_bytes(int64_t n_users, int64_t topn, int32_t n_slices) {
    if (n_users < 1 || topn < 1 || n_slices < 0) return 256;
    const int64_t s = n_slices == 0 ? WMF_RECOMMEND_AUTO_SLICES : n_slices;
    return WMF_RECOMMEND_WS_BASE + WMF_RECOMMEND_WS_PER_KEY * n_users * topn * s;
}

// the slices of a call: as many as give every CU two workgroups, at least WMF_REC_SLICE_TILES tiles each, the cap at most
int wmf_recommend_slices(int64_t n_users, int64_t n_items, int64_t topn, int32_t n_slices) {
    if (n_slices > 0) return n_slices;
    const int64_t blocks = (n_users + 16 * rec_waves(topn) - 1) / (16 * rec_waves(topn));
    const int64_t tiles = (n_items + 15) / 16;
    int64_t s = (2 * (int64_t)wmf_cu_count() + blocks - 1) / blocks;
    const int64_t by_tiles = (tiles + WMF_REC_SLICE_TILES - 1) / WMF_REC_SLICE_TILES;
    if (s > by_tiles) s = by_tiles;
    if (s > WMF_RECOMMEND_AUTO_SLICES) s = WMF_RECOMMEND_AUTO_SLICES;
    return (int)(s < 1 ? 1 : s);
}

void wmf_launch_topn_merge(const unsigned long long* partial, int64_t n_rows, int n_slices, int topn, int32_t* out_rows, float* out_scores,
                           int32_t* out_count, hipStream_t st) {
    int64_t grid = (n_rows + 3) / 4;
    if (grid > WMF_REC_MERGE_GRID) grid = WMF_REC_MERGE_GRID;
    WMF_LAUNCH("recommend_merge_kernel", recommend_merge_kernel, dim3((unsigned)grid), dim3(256), 0, st, partial, n_rows, n_slices, topn,
               out_rows, out_scores, out_count);
}

// every form of the LDS path; the list form cuts its slices and tiles from the n_cand positions
int wmf_launch_recommend(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users,
                         int64_t n_items, const WmfRowFilter& flt, int64_t n_cand, int64_t topn, int32_t n_slices, int32_t* out_items,
                         float* out_scores, int32_t* out_count, void* ws, hipStream_t st) {
    const int64_t n_scan = flt.cand_idx ? n_cand : n_items;
    WmfScanArgs a = {users, items, ld, bias, user_idx, n_users, n_scan, wmf_recommend_slices(n_users, n_scan, topn, n_slices), st};
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(ws);
    const int n = (int)topn, cap = rec_cap(topn);
    const int rc = wmf_dispatch_scan(ld, [&](auto nit, auto tps) {
        return wmf_dispatch_list<4, 2>(rec_waves(topn), [&](auto nw) {
            return wmf_dispatch_list<0, 1, 2>(rec_form(flt), [&](auto form) {
                constexpr int NIT = decltype(nit)::value, TPS = decltype(tps)::value, NW = decltype(nw)::value, FORM = decltype(form)::value;
                wmf_scan_geometry(a, NW);
                static const char* name = wmf_kname("recommend_scan_%skernel<%d, %d, %d>", REC_FORM_NAME[FORM], NIT, TPS, NW);
                WMF_LAUNCH_LDS(name, (recommend_scan_kernel<NIT, TPS, NW, FORM>), 112 * 1024, dim3((unsigned)a.grid), dim3(64 * NW),
                               wmf_scan_stage_bytes(TPS, ld) + rec_lds_bytes(NW, cap) + rec_form_lds(TPS, FORM), st, a.users, a.items, a.ld,
                               a.bias, a.user_idx, a.n_rows, a.n_items, WMF_FILTER_ARGS(flt), n, cap, a.n_slices, a.tiles_per_slice, a.n_work, partial);
                return (int)WMF_L_OK;
            });
        });
    });
    if (rc) return rc;
    wmf_launch_topn_merge(partial, n_users, a.n_slices, n, out_items, out_scores, out_count, st);
    return WMF_L_OK;
}

// ---- the wide launcher ------------------------------------------------------------------------------------------------------
// the lists -- (batch position, slice) pairs -- the workspace of an automatic call is sized for: monotone in n_users
static int64_t rec_wide_auto_lists(int64_t n_users) {
    const int64_t most = WMF_RECOMMEND_WIDE_AUTO_SLICES * n_users;
    const int64_t want = n_users > WMF_RECOMMEND_WIDE_AUTO_LISTS ? n_users : WMF_RECOMMEND_WIDE_AUTO_LISTS;
    return most < want ? most : want;
}
// (the lists of a call's workspace, for the scans of wmf_sample.hip that cut their slices alike)
int64_t wmf_recommend_wide_lists(int64_t n_users, int32_t n_slices) { return n_slices == 0 ? rec_wide_auto_lists(n_users) : n_users * n_slices; }
// ... and the slice count that fits them
static int64_t rec_wide_auto_bound(int64_t n_users) { return rec_wide_auto_lists(n_users) / n_users; }

int64_t wmf_recommend_wide_ws_bytes(int64_t n_users, int64_t topn, int32_t n_slices) {
    if (n_users < 1 || topn < 1 || n_slices < 0) return WMF_RECOMMEND_WIDE_WS_BASE;
    const int64_t lists = n_slices == 0 ? rec_wide_auto_lists(n_users) : n_users * n_slices;
    return WMF_RECOMMEND_WIDE_WS_BASE + lists * (WMF_RECOMMEND_WIDE_WS_PER_KEY * WMF_RECOMMEND_WIDE_CAP(topn) + WMF_RECOMMEND_WIDE_WS_PER_LIST);
}

// the slices of a wide call: the bound above, and a slice at least WMF_RECOMMEND_WIDE_SLICE_TOPNS x topn items (and
// WMF_REC_SLICE_TILES tiles) long, so that insertions -- about topn (1 + ln(slice / topn)) per row and slice -- stay rare
int wmf_recommend_wide_slices(int64_t n_users, int64_t n_scan, int64_t topn, int32_t n_slices) {
    if (n_slices > 0) return n_slices;
    const int64_t tiles = (n_scan + 15) / 16;
    int64_t slice_tiles = (WMF_RECOMMEND_WIDE_SLICE_TOPNS * topn + 15) / 16;
    if (slice_tiles < WMF_REC_SLICE_TILES) slice_tiles = WMF_REC_SLICE_TILES;
    int64_t s = rec_wide_auto_bound(n_users);
    const int64_t by_tiles = (tiles + slice_tiles - 1) / slice_tiles;
    if (s > by_tiles) s = by_tiles;
    return (int)(s < 1 ? 1 : s);
}

// What the launchers of the workspace buffers share: the workspace as [keys: n_virtual x n_slices buffers of cap][counts: one per
// buffer], scan(keys, counts, cap) -- the launcher's own scan, a WmfLaunchRc -- and the selection over the n_virtual rows.
template <class Scan>
static int rec_wide_scan_select(void* ws, int64_t n_virtual, int n_slices, int topn, int32_t* out_items, float* out_scores,
                                int32_t* out_count, hipStream_t st, Scan&& scan) {
    const int cap = WMF_RECOMMEND_WIDE_CAP(topn);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws);
    int32_t* counts = reinterpret_cast<int32_t*>(keys + (size_t)n_virtual * n_slices * cap);
    const int rc = scan(keys, counts, cap);
    if (rc) return rc;
    const int64_t grid = n_virtual < WMF_REC_MERGE_GRID ? n_virtual : WMF_REC_MERGE_GRID;    // rows beyond it take another trip
    WMF_LAUNCH("recommend_select_wide_kernel", recommend_select_wide_kernel, dim3((unsigned)grid), dim3(256), 0, st, keys, counts, n_virtual,
               n_slices, topn, cap, out_items, out_scores, out_count);
    return WMF_L_OK;
}

// any form of the filter
int wmf_launch_recommend_wide(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users,
                              int64_t n_items, const WmfRowFilter& flt, int64_t n_cand, int64_t topn, int32_t n_slices, int32_t* out_items,
                              float* out_scores, int32_t* out_count, void* ws, hipStream_t st) {
    const int64_t n_scan = flt.cand_idx ? n_cand : n_items;
    WmfScanArgs a = {users, items, ld, bias, user_idx, n_users, n_scan, wmf_recommend_wide_slices(n_users, n_scan, topn, n_slices), st};
    constexpr int NW = WMF_REC_WIDE_WAVES;
    wmf_scan_geometry(a, NW);
    return rec_wide_scan_select(ws, n_users, a.n_slices, (int)topn, out_items, out_scores, out_count, st, [&](auto* keys, auto* counts, int cap) {
        return wmf_dispatch_scan(ld, [&](auto nit, auto tps) {
            return wmf_dispatch_list<0, 1, 2>(rec_form(flt), [&](auto form) {
                constexpr int NIT = decltype(nit)::value, TPS = decltype(tps)::value, FORM = decltype(form)::value;
                static const char* name = wmf_kname("recommend_scan_wide_%skernel<%d, %d, %d>", REC_FORM_NAME[FORM], NIT, TPS, NW);
                WMF_LAUNCH_LDS(name, (recommend_scan_wide_kernel<NIT, TPS, NW, FORM>), 112 * 1024, dim3((unsigned)a.grid), dim3(64 * NW),
                               wmf_scan_stage_bytes(TPS, ld) + rec_wide_lds_bytes(NW) + rec_form_lds(TPS, FORM), st, a.users, a.items, a.ld,
                               a.bias, a.user_idx, a.n_rows, a.n_items, WMF_FILTER_ARGS(flt), (int)topn, cap, a.n_slices, a.tiles_per_slice, a.n_work, keys, counts);
                return (int)WMF_L_OK;
            });
        });
    });
}

// ---- the grouped launcher ---------------------------------------------------------------------------------------------------
int64_t wmf_recommend_grouped_ws_bytes(int64_t n_users, int32_t n_groups, int64_t topn, int32_t n_slices) {
    if (n_users < 1 || n_groups < 1 || topn < 1 || n_slices < 0) return WMF_RECOMMEND_WIDE_WS_BASE;
    const int64_t lists = n_slices == 0 ? rec_wide_auto_lists(n_users) : n_users * n_slices;
    return WMF_RECOMMEND_WIDE_WS_BASE +
           n_groups * lists * (WMF_RECOMMEND_WIDE_WS_PER_KEY * WMF_RECOMMEND_WIDE_CAP(topn) + WMF_RECOMMEND_WIDE_WS_PER_LIST);
}

// the slices of a grouped call: the wide rule with topn * n_groups for the minimum slice length (with even groups a slice then
// holds at least WMF_RECOMMEND_WIDE_SLICE_TOPNS x topn items of every group)
int wmf_recommend_grouped_slices(int64_t n_users, int64_t n_items, int32_t n_groups, int64_t topn, int32_t n_slices) {
    return wmf_recommend_wide_slices(n_users, n_items, topn * n_groups, n_slices);
}

// the mask form or no filter; the selection runs over the n_users * n_groups virtual rows
int wmf_launch_recommend_grouped(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users,
                                 int64_t n_items, const WmfRowFilter& flt, const int32_t* group_of, int32_t n_groups, int64_t topn,
                                 int32_t n_slices, int32_t* out_items, float* out_scores, int32_t* out_count, void* ws, hipStream_t st) {
    WmfScanArgs a = {users, items, ld, bias, user_idx, n_users, n_items, wmf_recommend_grouped_slices(n_users, n_items, n_groups, topn, n_slices), st};
    constexpr int NW = WMF_REC_WIDE_WAVES;
    wmf_scan_geometry(a, NW);
    return rec_wide_scan_select(ws, n_users * n_groups, a.n_slices, (int)topn, out_items, out_scores, out_count, st,
                                [&](auto* keys, auto* counts, int cap) {
        return wmf_dispatch_scan(ld, [&](auto nit, auto tps) {
            return wmf_dispatch_list<0, 1>(rec_form(flt), [&](auto form) {
                constexpr int NIT = decltype(nit)::value, TPS = decltype(tps)::value;
                constexpr bool MASK = decltype(form)::value == 1;
                static const char* name = wmf_kname("recommend_scan_grouped_%skernel<%d, %d, %d>", REC_FORM_NAME[MASK], NIT, TPS, NW);
                WMF_LAUNCH_LDS(name, (recommend_scan_grouped_kernel<NIT, TPS, NW, MASK>), 112 * 1024, dim3((unsigned)a.grid), dim3(64 * NW),
                               wmf_scan_stage_bytes(TPS, ld) + rec_grouped_lds_bytes(NW, n_groups), st, a.users, a.items, a.ld, a.bias, a.user_idx,
                               a.n_rows, a.n_items, WMF_FILTER_ARGS(flt), group_of, (int)n_groups, (int)topn, cap, a.n_slices, a.tiles_per_slice, a.n_work, keys,
                               counts);
                return (int)WMF_L_OK;
            });
        });
    });
}
