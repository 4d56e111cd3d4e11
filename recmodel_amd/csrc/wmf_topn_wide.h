// The running top-n of a catalogue scan beyond what LDS holds (gfx950): the epilogue policy of wmf_recommend_topn_wide, 1 <= topn <=
// WMF_RECOMMEND_WIDE_MAX_TOPN.  A row's keys live in the WORKSPACE, one buffer of `cap` keys per (batch position, slice) pair; counts
// and thresholds stay in LDS and registers as in RecTopN (wmf_topn.h).  A buffer that the next tile could overflow is cut back to its
// topn best by an exact radix select of the topn-th largest key (the keys of a row are pairwise distinct, so that key is unique) and
// one in-place compaction pass (rec_wide_cut_buffer, which RecTopNGrouped calls too); nothing is sorted during the scan.
// recommend_select_wide_kernel (wmf_recommend.hip) selects and sorts the topn best of a row's slices with the same select.
//
// Who owns what: one wave owns the buffers of its 16 rows for the whole launch, and no other wave of the grid reads or writes them
// before the kernel ends.  What orders the wave's own global accesses: see rec_wide_drain.
#pragma once
#include "wmf_scan.h"
#include "wmf_filter.h"

// A lane's global store followed by ANOTHER lane's load of the same address, both of one wave.  A wave issues its vector-memory
// instructions in program order and all of them go through the one vector L1 of its CU, which writes through to L2; VM_CNT counts a
// store until L2 has acknowledged it.  The load below the wait is therefore issued after the data is in L2 and after the L1 has seen
// the store (the LLVM memory model for gfx942/gfx950 needs no cache action at wavefront or workgroup scope for that reason); the
// fences keep the compiler from moving an access across.  wmf_wave_sync alone waits for nothing on the vector-memory side.
__device__ __forceinline__ void rec_wide_drain() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The k-th largest (k = 1: the largest) of the keys of n_seg segments, segment s = base[s * seg_stride ...] of seg_cnt[s] keys
// (seg_cnt == NULL: one segment of n_single keys); 1 <= k <= the number of keys, the keys pairwise distinct.  Eight passes over the
// keys, most significant byte first: a 256-bin histogram (LDS atomics, integers: any order gives the same counts) of the keys that
// share the prefix found so far, then the bin that holds the k-th.  Called by NT threads together, t = the thread's index among them;
// NT = 64: one wave, hist is that wave's; NT > 64: the workgroup, one hist, __syncthreads.  Every thread returns the key.
template <int NT>
__device__ __forceinline__ void rec_wide_sync() {
    if constexpr (NT == 64) wmf_wave_sync(); else __syncthreads();
}
template <int NT>
__device__ __forceinline__ unsigned long long rec_wide_kth(const unsigned long long* base, const int32_t* seg_cnt, int n_seg,
                                                           int64_t seg_stride, int n_single, int seg_max, int k, unsigned* hist, int t) {
    const int lane = t & 63;
    unsigned long long prefix = 0ull, mask = 0ull;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = t; i < 256; i += NT) hist[i] = 0u;
        rec_wide_sync<NT>();
        for (int s = 0; s < n_seg; ++s) {
            const unsigned long long* seg = base + s * seg_stride;
            const int c = seg_cnt ? min(seg_cnt[s], seg_max) : n_single;
            for (int e = t; e < c; e += NT) {
                const unsigned long long key = seg[e];
                if ((key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
        }
        rec_wide_sync<NT>();
        // every wave for itself: lane l holds bins 4 l .. 4 l + 3; above = the keys in the bins of the higher lanes
        const unsigned h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const int own = (int)(h0 + h1 + h2 + h3);
        int incl = own;                                            // own + the higher lanes'
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_down(incl, o);
            if (lane + o < 64) incl += v;
        }
        const int above = incl - own;
        const bool here = above < k && k <= incl;                  // exactly one lane
        int bin = 0, k_next = 0;
        if (here) {
            int a = above;
            if (k <= a + (int)h3) { bin = 4 * lane + 3; }
            else if (a += (int)h3, k <= a + (int)h2) { bin = 4 * lane + 2; }
            else if (a += (int)h2, k <= a + (int)h1) { bin = 4 * lane + 1; }
            else { a += (int)h1; bin = 4 * lane; }
            k_next = k - a;
        }
        const int src = __builtin_ctzll(__ballot(here) | (1ull << 63));
        bin = __shfl(bin, src);
        k = __shfl(k_next, src);
        prefix |= (unsigned long long)(unsigned)bin << shift;
        mask |= 255ull << shift;
        rec_wide_sync<NT>();                                       // the bins are read before the next pass clears them
    }
    return prefix;
}

// A buffer of n keys (n <= cap) cut back, in place, to its topn best, by one wave: the topn-th largest key T (returned), then the keys
// >= T moved to the front, 64 at a time.  THE overwrite argument of every in-place cut: a chunk is loaded before any of its keys is
// stored (the store's data depends on the load), and it is stored at or below where it was read, so no key is overwritten before it
// is read.  The caller drains (rec_wide_drain) before -- the keys other lanes appended -- and after, and keeps the count and threshold.
__device__ __forceinline__ unsigned long long rec_wide_cut_buffer(unsigned long long* ku, int n, int cap, int topn, unsigned* hist, int lane) {
    const unsigned long long T = rec_wide_kth<64>(ku, nullptr, 1, 0, n, cap, topn, hist, lane);
    int out = 0;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const unsigned long long key = e0 + lane < n ? ku[e0 + lane] : 0ull;
        const bool keep = key >= T && e0 + lane < n;
        const unsigned long long m = __ballot(keep);
        if (keep) ku[out + __popcll(m & ((1ull << lane) - 1ull))] = key;
        out += __popcll(m);
    }
    return T;
}

// The topn best keys of all of a row's slices -- K: the row's n_slices buffers of cap keys as the scan left them, C: their counts --
// sorted best first into sel (LDS, WMF_RECOMMEND_WIDE_MAX_TOPN keys): the exact select above over the buffers, then a bitonic sort
// (the keys are distinct: one result).  By the 256 threads of a workgroup together, t the thread; hist: 256 words and counters: two
// ints of LDS.  Every thread returns the number of keys, min(topn, the row's keys); the caller holds a barrier between its reads of
// sel and the next row.  What recommend_select_wide_kernel (wmf_recommend.hip) and sample_select_kernel (wmf_sample.hip) share.
__device__ __forceinline__ int rec_wide_select_row(const unsigned long long* __restrict__ K, const int32_t* __restrict__ C, int n_slices,
                                                   int topn, int cap, unsigned long long* sel, unsigned* hist, int* counters, int t) {
    int& total_s = counters[0];
    int& fill_s = counters[1];
    if (t == 0) { total_s = 0; fill_s = 0; }
    __syncthreads();
    int mine = 0;
    for (int s = t; s < n_slices; s += 256) mine += min(C[s], cap);
    if (mine) atomicAdd(&total_s, mine);
    __syncthreads();
    const int m = total_s, count = min(m, topn);                   // (uniform: the select below holds barriers)
    unsigned long long T = 1ull;                                   // every key of an item is above 0
    if (m > topn) T = rec_wide_kth<256>(K, C, n_slices, cap, 0, cap, topn, hist, t);
    int P = 1;
    while (P < count) P <<= 1;
    for (int i = t; i < P; i += 256) sel[i] = 0ull;
    __syncthreads();
    for (int s = 0; s < n_slices; ++s) {
        const int c = min(C[s], cap);
        for (int e = t; e < c; e += 256) {
            const unsigned long long key = K[(size_t)s * cap + e];
            if (key >= T) {
                const int slot = atomicAdd(&fill_s, 1);            // exactly `count` keys are at or above T
                if (slot < topn) sel[slot] = key;
            }
        }
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < P; i += 256) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long x = sel[i], y = sel[o];
                    if ((i & k) == 0 ? x < y : x > y) { sel[i] = y; sel[o] = x; }
                }
            }
            __syncthreads();
        }
    }
    return count;
}

// The scan's epilogue.  Workspace: keys[(b * n_slices + slice) * cap + e], e < counts[b * n_slices + slice], in no order, the topn
// best eligible keys of that slice among them.  LDS past the stages: [thresholds: 16 per wave, 8 B][counts: 16 per wave][histogram:
// 256 per wave].  MASK as in RecTopN.
template <int NW, bool MASK = false>
struct RecTopNWide {
    WmfRowFilter filter;
    int64_t n_users; int topn, cap, n_slices;
    unsigned long long* keys_ws; int32_t* counts_ws;              // (not restrict: lanes read what other lanes of the wave wrote)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    unsigned long long* thr_l; int* cnt; unsigned* hist;
    int64_t u0; int sl;
    unsigned long long thr[4];
    unsigned long long* buf0; int64_t row_stride;                  // the buffer of row u0 + 4 q + reg: buf0 + reg * row_stride
    WmfRowEligible<false, MASK> ok;

    __device__ __forceinline__ unsigned long long* row_buf(int64_t b) const { return keys_ws + ((size_t)b * n_slices + sl) * (size_t)cap; }
    __device__ __forceinline__ void begin(unsigned char* lds, int64_t u0_, int sl_) {
        u0 = u0_; sl = sl_;
        thr_l = reinterpret_cast<unsigned long long*>(lds) + wave * 16;
        cnt = reinterpret_cast<int*>(lds + (size_t)NW * 16 * 8) + wave * 16;
        hist = reinterpret_cast<unsigned*>(lds + (size_t)NW * 16 * 12) + wave * 256;
        if (lane < 16) { cnt[lane] = 0; thr_l[lane] = 0ull; }
        buf0 = row_buf(u0 + 4 * q);                                // (rows past the batch: never dereferenced)
        row_stride = (int64_t)n_slices * cap;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) thr[reg] = 0ull;
        ok.begin(filter, u0, q, n_users);
        wmf_wave_sync();
    }
    __device__ __forceinline__ void score(int reg, int, int64_t item, unsigned long long key, bool in_range) {
        if (in_range && u0 + 4 * q + reg < n_users && key > thr[reg] && ok.pass(reg, item)) {
            const int slot = atomicAdd(&cnt[4 * q + reg], 1);      // at most 16 per row and tile: below cap
            if (slot < cap) buf0[reg * row_stride + slot] = key;
        }
    }
    // The buffers of the wave's rows in `full` (bit u = row u of 16) cut back to their topn best (rec_wide_cut_buffer)
    __device__ __forceinline__ void cut(unsigned full) {
        rec_wide_drain();                                          // the keys other lanes appended
        while (full) {
            const int u = __builtin_ctz(full);
            full &= full - 1;
            const unsigned long long T = rec_wide_cut_buffer(row_buf(u0 + u), min(cnt[u], cap), cap, topn, hist, lane);
            if (lane == 0) { cnt[u] = topn; thr_l[u] = T; }
        }
        rec_wide_drain();                                          // the compacted keys before the next appends and the next cut
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) thr[reg] = thr_l[4 * q + reg];
    }
    __device__ __forceinline__ void tile(int) {
        wmf_wave_sync();
        const unsigned full = (unsigned)(__ballot(cnt[r] > cap - 16) & 0xFFFFull);
        if (full) cut(full);
    }
    __device__ __forceinline__ void end() {
        wmf_wave_sync();
        if (lane < 16 && u0 + lane < n_users) counts_ws[(u0 + lane) * n_slices + sl] = min(cnt[lane], cap);
        wmf_wave_sync();                                           // the counts are read before the next pair resets them
    }
};

// ---- sizes ------------------------------------------------------------------------------------------------------------------
#define WMF_REC_WIDE_WAVES 4                                       /* waves of a wide scan's workgroup: one value, no switch */
// (the keys of a buffer: WMF_RECOMMEND_WIDE_CAP(topn) of include/wmf_hip.h, >= topn + 16)
// dynamic LDS of a scan with this epilogue, past the stages
__host__ __device__ static inline size_t rec_wide_lds_bytes(int nw) { return (size_t)nw * 16 * 12 + (size_t)nw * 256 * 4; }
