// The running top-n of a catalogue scan (gfx950): the epilogue policy that wmf_recommend.hip and wmf_similar.hip hand to
// wmf_catalogue_scan, and the sizes of its LDS buffers.  The partial lists it writes are merged by recommend_merge_kernel
// (wmf_recommend.hip, wmf_launch_topn_merge).
#pragma once
#include "wmf_scan.h"

// The buffers of the wave's users in `mask` (bit u = user u of 16) cut back to their topn best, sorted best first; thr[u] = the
// topn-th best once there are that many.  A key's place is the number of keys above it (the keys are distinct): every lane
// holds up to four keys of the buffer (cap <= 256) and counts against broadcast reads of all of them.
__device__ __forceinline__ void rec_compact(unsigned mask, unsigned long long* __restrict__ keys, int* __restrict__ cnt,
                                            unsigned long long* __restrict__ thr, int cap, int topn, int lane) {
    while (mask) {
        const int u = __builtin_ctz(mask);
        mask &= mask - 1;
        unsigned long long* ku = keys + u * cap;
        const int n = min(cnt[u], cap);
        unsigned long long e[4];
        int place[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            e[k] = (lane + 64 * k < n) ? ku[lane + 64 * k] : 0ull;
            place[k] = 0;
        }
        for (int j = 0; j < n; ++j) {
            const unsigned long long o = ku[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) place[k] += (o > e[k]) ? 1 : 0;
        }
        wmf_wave_sync();                                           // every read of the buffer before the first write
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (lane + 64 * k < n && place[k] < topn) {
                ku[place[k]] = e[k];
                if (place[k] == topn - 1) thr[u] = e[k];
            }
        }
        if (lane == 0) cnt[u] = min(n, topn);
        wmf_wave_sync();
    }
}

// The scan's epilogue: a running top-n per user.  LDS past the stages: [keys: 16 users x cap per wave][thresholds][counts].
// partial[(b * n_slices + slice) * topn + k]: the k-th best key of batch position b in that slice, 0 = none.
// SELF: the row's own id (self_idx[b], the catalogue row that batch position b is) is never inserted; self_idx == NULL: no such row.
// MASK: an allow mask per row, allow_bits[allow_idx[b]][allow_words] (allow_idx == NULL: mask 0 for every row; allow_idx[b] == -1:
// row b has none): item j may be inserted only when bit j & 31 of word j >> 5 is set.  Tested at insertion, after the threshold and
// before the seen list (one load against the search's twenty): a masked-out item never enters a buffer or raises a threshold.
template <int NW, bool SELF = false, bool MASK = false>
struct RecTopN {
    const int64_t* __restrict__ seen_indptr; const int32_t* __restrict__ seen_indices;
    int64_t n_users; int topn, cap, n_slices;
    unsigned long long* __restrict__ partial;
    const int32_t* __restrict__ self_idx = nullptr;               // (self_idx and self[] are dead without SELF: the kernels' code is the same)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    unsigned long long* keys; unsigned long long* thr_l; int* cnt;
    int64_t u0; int sl;
    unsigned long long thr[4];
    int64_t seen_lo[4], seen_hi[4];
    int32_t self[4];
    // (MASK; set by the kernel after the aggregate's members above, and dead without MASK like self[])
    const uint32_t* __restrict__ allow_bits = nullptr; int64_t allow_words = 0; const int32_t* __restrict__ allow_idx = nullptr;
    const uint32_t* words[4];

    __device__ __forceinline__ void begin(unsigned char* lds, int64_t u0_, int sl_) {
        u0 = u0_; sl = sl_;
        keys = reinterpret_cast<unsigned long long*>(lds) + (size_t)wave * 16 * cap;
        thr_l = reinterpret_cast<unsigned long long*>(lds) + (size_t)NW * 16 * cap + wave * 16;
        cnt = reinterpret_cast<int*>(lds + ((size_t)NW * 16 * cap + NW * 16) * 8) + wave * 16;
        if (lane < 16) { cnt[lane] = 0; thr_l[lane] = 0ull; }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            thr[reg] = 0ull; seen_lo[reg] = 0; seen_hi[reg] = 0;
            const int64_t b = u0 + 4 * q + reg;
            if (seen_indptr && b < n_users) { seen_lo[reg] = seen_indptr[b]; seen_hi[reg] = seen_indptr[b + 1]; }
            if constexpr (SELF) self[reg] = (self_idx && b < n_users) ? self_idx[b] : -1;
            if constexpr (MASK) {
                const int32_t g = b < n_users ? (allow_idx ? allow_idx[b] : 0) : -1;
                words[reg] = g >= 0 ? allow_bits + (int64_t)g * allow_words : nullptr;
            }
        }
        wmf_wave_sync();
    }
    // A key that beats the user's threshold is looked up in the user's sorted seen list and, if it is not there, appended
    __device__ __forceinline__ void score(int reg, int, int64_t item, unsigned long long key, bool in_range) {
        bool take = in_range && u0 + 4 * q + reg < n_users && key > thr[reg];
        if constexpr (SELF) take = take && (int32_t)item != self[reg];
        if constexpr (MASK) {
            if (take && words[reg]) take = (words[reg][item >> 5] >> (item & 31)) & 1u;
        }
        if (take && seen_lo[reg] < seen_hi[reg]) {
            int64_t lo = seen_lo[reg], hi = seen_hi[reg];
            while (lo < hi) {                                      // first entry >= item
                const int64_t mid = (lo + hi) >> 1;
                if (seen_indices[mid] < (int32_t)item) lo = mid + 1; else hi = mid;
            }
            take = !(lo < seen_hi[reg] && seen_indices[lo] == (int32_t)item);
        }
        if (take) {
            const int slot = atomicAdd(&cnt[4 * q + reg], 1);      // at most 16 per user and tile: below cap
            if (slot < cap) keys[(4 * q + reg) * cap + slot] = key;
        }
    }
    // a buffer the next tile could overflow is cut back to its topn best
    __device__ __forceinline__ void tile(int) {
        wmf_wave_sync();
        const unsigned full = (unsigned)(__ballot(cnt[r] > cap - 16) & 0xFFFFull);
        if (full) {
            rec_compact(full, keys, cnt, thr_l, cap, topn, lane);
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) thr[reg] = thr_l[4 * q + reg];
        }
    }
    __device__ __forceinline__ void end() {
        rec_compact((unsigned)(__ballot(cnt[r] > 0) & 0xFFFFull), keys, cnt, thr_l, cap, topn, lane);
        for (int u = 0; u < 16 && u0 + u < n_users; ++u) {
            unsigned long long* out = partial + ((u0 + u) * n_slices + sl) * topn;
            const int n = cnt[u];
            for (int k = lane; k < topn; k += 64) out[k] = k < n ? keys[u * cap + k] : 0ull;
        }
        wmf_wave_sync();                                           // the buffers are read before the next pair resets them
    }
};

// ---- sizes ------------------------------------------------------------------------------------------------------------------
static inline int rec_cap(int64_t topn) { return (int)(2 * topn > 32 ? 2 * topn : 32); }       // >= topn + 16, <= 256
static inline int rec_waves(int64_t topn) { return rec_cap(topn) <= 128 ? 4 : 2; }               // 64 KB of key buffers at most
// dynamic LDS of a scan with this epilogue, past the stages: the key buffers, thresholds and counts of 16 NW rows
__host__ __device__ static inline size_t rec_lds_bytes(int nw, int cap) { return ((size_t)nw * 16 * cap + nw * 16) * 8 + (size_t)nw * 16 * 4; }
