// The running top-n of EVERY GROUP of a catalogue scan (gfx950): the epilogue policy of wmf_recommend_topn_grouped.  group_of[j] is
// the group (shelf) of item j; a row keeps one key buffer per (group, slice) in the workspace, so one scan of the catalogue answers
// n_groups questions per row and every score is computed once.  The machinery is RecTopNWide's (wmf_topn_wide.h) over the virtual
// rows v = b * n_groups + g: keys[(v * n_slices + slice) * cap + e], counts[v * n_slices + slice] -- the layout
// recommend_select_wide_kernel reads for n_users * n_groups rows.  Thresholds and counts of the wave's 16 x n_groups buffers live in
// LDS (a lane's four scores of a tile are four rows against ONE item, hence one group id per lane and tile, and the threshold is
// read where a register held it in RecTopNWide).
//
// The overflow bound carries over: a tile adds at most 16 keys to a row, hence at most 16 to any one of the row's buffers, so a buffer
// holding <= cap - 16 keys before a tile cannot overflow within it.  A lane whose append returns a slot >= cap - 16 (the count has
// passed cap - 16) marks its (row, group); after the tile the wave cuts every marked buffer back to its topn best (<= cap - 16) with
// rec_wide_cut_buffer (wmf_topn_wide.h: the select and the in-place compaction), re-checking the count so that a buffer marked by several lanes is cut once.
// Who owns what is unchanged: one wave owns all buffers of its 16 rows for the whole work unit.
//
// The group ids travel one stage ahead of their tiles: at the first tile of a stage, lane (r, q) asks for the id of item row r of
// the NEXT stage's tile q mod TPS (one coalesced read of 16 TPS ids, clamped to the catalogue), and the ids of the stage at hand are the
// ones asked for a stage ago, handed to the tile's lanes by a shuffle.  Only the first stage of a work unit waits for its read.
#pragma once
#include "wmf_topn_wide.h"

// LDS past the stages: [thresholds: 16 n_groups per wave, 8 B][counts: 16 n_groups per wave][histogram: 256 per wave].  MASK as in
// RecTopN.  TPS: the scan's tiles per stage.
template <int TPS, int NW, bool MASK = false>
struct RecTopNGrouped {
    WmfRowFilter filter;
    int64_t n_users; int topn, cap, n_slices;
    unsigned long long* keys_ws; int32_t* counts_ws;              // (not restrict: lanes read what other lanes of the wave wrote)
    const int32_t* __restrict__ group_of; int64_t n_items; int n_groups;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    unsigned long long* thr_l; int* cnt; unsigned* hist;
    int64_t u0; int sl;
    unsigned long long* buf0; int64_t row_stride, group_stride;    // the buffer of (row u0 + 4 q + reg, group g): buf0 + reg * row_stride + g * group_stride
    WmfRowEligible<false, MASK> ok;
    int32_t gvec, gpre; int64_t pre_base;                          // the ids of this stage's tiles and of the next one's, and where those start
    int32_t g; unsigned marked;                                    // this tile: the lane's group id; bit reg: (row 4 q + reg, g) has passed cap - 16

    __device__ __forceinline__ unsigned long long* row_buf(int64_t b, int grp) const {
        return keys_ws + (((size_t)b * n_groups + grp) * n_slices + sl) * (size_t)cap;
    }
    __device__ __forceinline__ void begin(unsigned char* lds, int64_t u0_, int sl_) {
        u0 = u0_; sl = sl_;
        const int per_wave = 16 * n_groups;
        thr_l = reinterpret_cast<unsigned long long*>(lds) + wave * per_wave;
        cnt = reinterpret_cast<int*>(lds + (size_t)NW * per_wave * 8) + wave * per_wave;
        hist = reinterpret_cast<unsigned*>(lds + (size_t)NW * per_wave * 12) + wave * 256;
        for (int i = lane; i < per_wave; i += 64) { cnt[i] = 0; thr_l[i] = 0ull; }
        group_stride = (int64_t)n_slices * cap;
        row_stride = group_stride * n_groups;
        buf0 = row_buf(u0 + 4 * q, 0);                             // (rows past the batch: never dereferenced)
        pre_base = -1; gvec = -1; gpre = -1; g = -1; marked = 0u;
        ok.begin(filter, u0, q, n_users);
        wmf_wave_sync();
    }
    // the group id of this lane's item of the stage's j-th tile (item = 16 tile + r: this policy has no list form)
    __device__ __forceinline__ void fetch(int j, int64_t item) {
        if (j == 0) {                                              // every stage has its tile 0
            const int64_t base = item - r, last = n_items - 1;
            const int t = q % TPS;                                 // the tile this lane asks for (TPS = 1: every lane its own tile's)
            if (base != pre_base) gpre = group_of[min(base + 16 * t + r, last)];    // the first stage of a work unit
            gvec = gpre;
            gpre = group_of[min(base + 16 * (TPS + t) + r, last)];
            pre_base = base + 16 * TPS;
        }
        g = TPS == 1 ? gvec : __shfl(gvec, 16 * j + r);
    }
    __device__ __forceinline__ void score(int reg, int j, int64_t item, unsigned long long key, bool in_range) {
        if (reg == 0) fetch(j, item);
        bool take = in_range && u0 + 4 * q + reg < n_users && (unsigned)g < (unsigned)n_groups;   // unsigned: -1 and its like are no shelf
        const int li = (4 * q + reg) * n_groups + (take ? g : 0);
        if (take && key > thr_l[li] && ok.pass(reg, item)) {       // (the buffer's threshold lives in LDS: one per (row, group))
            const int slot = atomicAdd(&cnt[li], 1);               // at most 16 per buffer and tile: below cap
            if (slot < cap) buf0[reg * row_stride + g * group_stride + slot] = key;
            if (slot >= cap - 16) marked |= 1u << reg;
        }
    }
    // The buffers the lanes of `who` marked, cut back to their topn best (rec_wide_cut_buffer); the new threshold goes to LDS.
    __device__ __forceinline__ void cut(unsigned long long who) {
        rec_wide_drain();                                          // the keys other lanes appended
        while (who) {
            const int src = __builtin_ctzll(who);
            who &= who - 1;
            unsigned m = (unsigned)__builtin_amdgcn_readlane((int)marked, src);
            const int grp = __builtin_amdgcn_readlane(g, src);
            while (m) {
                const int u = 4 * (src >> 4) + __builtin_ctz(m);
                m &= m - 1;
                const int li = u * n_groups + grp;
                const int have = __builtin_amdgcn_readfirstlane(cnt[li]);
                if (have <= cap - 16) continue;                    // another lane marked it too: it is cut already
                const unsigned long long T = rec_wide_cut_buffer(row_buf(u0 + u, grp), min(have, cap), cap, topn, hist, lane);
                if (lane == 0) { cnt[li] = topn; thr_l[li] = T; }
                wmf_wave_sync();                                   // the count before the next look at it
            }
        }
        rec_wide_drain();                                          // the compacted keys before the next appends and the next cut
    }
    __device__ __forceinline__ void tile(int) {
        wmf_wave_sync();
        const unsigned long long who = __ballot(marked != 0u);
        if (who) cut(who);
        marked = 0u;
    }
    __device__ __forceinline__ void end() {
        wmf_wave_sync();
        const int64_t left = n_users - u0;
        const int n = (int)(left < 16 ? left : 16) * n_groups;     // the counts of all the unit's buffers: a group that got nothing has 0
        for (int i = lane; i < n; i += 64) counts_ws[(u0 * n_groups + i) * n_slices + sl] = min(cnt[i], cap);
        wmf_wave_sync();                                           // the counts are read before the next pair resets them
    }
};

// dynamic LDS of a scan with this epilogue, past the stages: 768 B per group and workgroup of four waves, and the histograms
__host__ __device__ static inline size_t rec_grouped_lds_bytes(int nw, int n_groups) {
    return (size_t)nw * 16 * n_groups * 12 + (size_t)nw * 256 * 4;
}
