// The running top-n of a catalogue scan (gfx950): the epilogue policy that wmf_recommend.hip and wmf_similar.hip hand to
// wmf_catalogue_scan, and the sizes of its LDS buffers.  The partial lists it writes are merged by recommend_merge_kernel
// (wmf_recommend.hip, wmf_launch_topn_merge).  Which keys may enter a list, and in what order that is tested, is wmf_filter.h's;
// the epilogues here and in wmf_topn_wide.h / wmf_topn_grouped.h compare with their threshold and ask WmfRowEligible::pass.
#pragma once
#include "wmf_scan.h"
#include "wmf_filter.h"

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
// SELF, MASK: the tests of WmfRowEligible (wmf_filter.h) this instantiation runs besides the seen list; without them its code is
// that of the plain kernel.
template <int NW, bool SELF = false, bool MASK = false>
struct RecTopN {
    WmfRowFilter filter;
    int64_t n_users; int topn, cap, n_slices;
    unsigned long long* __restrict__ partial;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    unsigned long long* keys; unsigned long long* thr_l; int* cnt;
    int64_t u0; int sl;
    unsigned long long thr[4];
    WmfRowEligible<SELF, MASK> ok;

    __device__ __forceinline__ void begin(unsigned char* lds, int64_t u0_, int sl_) {
        u0 = u0_; sl = sl_;
        keys = reinterpret_cast<unsigned long long*>(lds) + (size_t)wave * 16 * cap;
        thr_l = reinterpret_cast<unsigned long long*>(lds) + (size_t)NW * 16 * cap + wave * 16;
        cnt = reinterpret_cast<int*>(lds + ((size_t)NW * 16 * cap + NW * 16) * 8) + wave * 16;
        if (lane < 16) { cnt[lane] = 0; thr_l[lane] = 0ull; }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) thr[reg] = 0ull;
        ok.begin(filter, u0, q, n_users);
        wmf_wave_sync();
    }
    // A key that beats the user's threshold and passes the filter is appended
    __device__ __forceinline__ void score(int reg, int, int64_t item, unsigned long long key, bool in_range) {
        if (in_range && u0 + 4 * q + reg < n_users && key > thr[reg] && ok.pass(reg, item)) {
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
