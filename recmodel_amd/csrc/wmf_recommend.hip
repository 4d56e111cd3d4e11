// Full-catalogue top-N with per-user exclusions (gfx950): the N best items of [0, n_items) for every user of a batch, leaving out
// what the user has seen -- the query of RecModel/utils.py:3-17 (test_coverage ranks np.delete(arange(n_items), seen) for every
// user) through WMF.rank (RecModel/wmf_model.py:25-47), in one fused pass: nothing of size n_users x n_items exists anywhere.
//
//   * recommend_scan_kernel  -- a workgroup holds 16 users per wave in registers (the operand pattern and bias rule of
//                               score_tile_kernel, wmf_rank.hip: bit-identical scores) and walks a contiguous SLICE of the
//                               catalogue's 16-item tiles, which it stages once in LDS for all its waves.  Every score becomes
//                               a 64-bit key (order-preserving key of the score, ~item id): ONE total order, a higher score wins,
//                               equal scores go to the lower id.  A key that beats the user's threshold -- the current N-th
//                               best -- is looked up in the user's sorted seen list (binary search) and, if it is not there,
//                               appended to the user's LDS buffer; a buffer that could overflow on the next tile is cut back to
//                               its N best, which also raises the threshold.  Insertions are rare (about N ln(n / N) per user),
//                               so neither the exclusion nor the selection costs anything in the scoring loop.
//   * recommend_merge_kernel -- the sorted partial lists of a user's slices merged by rank: a key's place is the number of
//                               keys above it, found by one binary search per slice.
// The keys of a user are pairwise distinct, so the result is a function of the scores alone: it cannot depend on the number of
// slices, the grid or the order in which workgroups, waves or LDS atomics finish.  No float atomics.

#include "wmf_common.h"
#include "wmf_internal.h"

#define WMF_REC_SCAN_GRID 4096       /* workgroups of the scan: (user block, slice) pairs beyond it take another trip */
#define WMF_REC_MERGE_GRID 1024      /* workgroups of the merge, four users each */
#define WMF_REC_SLICE_TILES 64       /* an automatic slice holds at least this many 16-item tiles */

// rank_key of wmf_rank.hip (ascending in the float order) with -0.0 = +0.0
__device__ __forceinline__ uint32_t rec_key(float s) {
    uint32_t u = __builtin_bit_cast(uint32_t, s);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rec_unkey(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
__device__ __forceinline__ void rec_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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
        rec_wave_sync();                                           // every read of the buffer before the first write
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (lane + 64 * k < n && place[k] < topn) {
                ku[place[k]] = e[k];
                if (place[k] == topn - 1) thr[u] = e[k];
            }
        }
        if (lane == 0) cnt[u] = min(n, topn);
        rec_wave_sync();
    }
}

// NIT: trips of the feature loop a wave can hold a user row for (4 NIT pieces of 16 bytes per row); TPS: 16-item tiles per stage.
// Dynamic LDS: [two stages of TPS x 16 item rows, (nch | 1) pieces apart][keys: 16 users x cap per wave][thresholds][counts].
// partial[(b * n_slices + slice) * topn + k]: the k-th best key of batch position b in that slice, 0 = none.
template <int NIT, int TPS>
__global__ __launch_bounds__(256) void recommend_scan_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld,
                                                             int bias, const int32_t* __restrict__ user_idx, int64_t n_users,
                                                             int64_t n_items, const int64_t* __restrict__ seen_indptr,
                                                             const int32_t* __restrict__ seen_indices, int topn, int cap,
                                                             int n_slices, int64_t tiles_per_slice, int64_t n_work,
                                                             unsigned long long* __restrict__ partial) {
    extern __shared__ __align__(16) unsigned char rec_smem[];
    constexpr int PRE = (TPS * NIT + 1) / 2;                      // 16-byte pieces of a stage per thread, at 128 threads
    const int nthreads = blockDim.x, nw = nthreads >> 6, tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2, nit = (nch + 3) >> 2, stride = nch | 1;
    const int stage_f4 = TPS * 16 * stride;
    float4* stage = reinterpret_cast<float4*>(rec_smem);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(rec_smem + (size_t)2 * stage_f4 * 16) + (size_t)wave * 16 * cap;
    unsigned long long* thr_l = reinterpret_cast<unsigned long long*>(rec_smem + (size_t)2 * stage_f4 * 16) + (size_t)nw * 16 * cap + wave * 16;
    int* cnt = reinterpret_cast<int*>(rec_smem + (size_t)2 * stage_f4 * 16 + ((size_t)nw * 16 * cap + nw * 16) * 8) + wave * 16;
    const float4* items4 = reinterpret_cast<const float4*>(items);
    const int64_t tiles = (n_items + 15) >> 4;

    // this thread's pieces of a stage: (item row of the stage) << 8 | piece
    int pk[PRE];
#pragma unroll
    for (int k = 0; k < PRE; ++k) {
        const int idx = tid + k * nthreads;
        pk[k] = idx < TPS * 16 * nch ? ((idx / nch) << 8) | (idx % nch) : -1;
    }

    for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int64_t ub = w / n_slices;
        const int sl = (int)(w % n_slices);
        const int64_t u0 = (ub * nw + wave) * 16;                  // first batch position of this wave
        const bool active = u0 < n_users;
        const int64_t t0 = min((int64_t)sl * tiles_per_slice, tiles), t1 = min(t0 + tiles_per_slice, tiles);
        const int64_t n_st = (t1 - t0 + TPS - 1) / TPS;

        // the wave's 16 user rows, for the whole scan: lane (r, q) holds pieces 4 it + q of user r
        float4 ureg[NIT];
        float ubr[4] = {0.f, 0.f, 0.f, 0.f};
        {
            const float4* urow = reinterpret_cast<const float4*>(users + (int64_t)user_idx[min(u0 + r, n_users - 1)] * ld);
            float ubv = 0.f;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = 4 * it + q;
                ureg[it] = (it < nit && c < nch) ? urow[c] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            if (bias && q == 0) { ubv = ureg[0].x; ureg[0].x = 0.f; }
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) ubr[reg] = __shfl(ubv, 4 * q + reg);    // user bias of user 4 q + reg
        }
        if (lane < 16) { cnt[lane] = 0; thr_l[lane] = 0ull; }
        unsigned long long thr[4] = {0ull, 0ull, 0ull, 0ull};
        int64_t seen_lo[4] = {0, 0, 0, 0}, seen_hi[4] = {0, 0, 0, 0};
        if (seen_indptr) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t b = u0 + 4 * q + reg;
                if (b < n_users) { seen_lo[reg] = seen_indptr[b]; seen_hi[reg] = seen_indptr[b + 1]; }
            }
        }
        rec_wave_sync();

        float4 pre[PRE];
        auto load_stage = [&](int64_t tile_first) {
#pragma unroll
            for (int k = 0; k < PRE; ++k) {
                if (pk[k] >= 0) {
                    const int64_t gi = min(16 * tile_first + (pk[k] >> 8), n_items - 1);       // clamped: the scores are masked
                    pre[k] = items4[gi * nch + (pk[k] & 255)];
                }
            }
        };
        auto store_stage = [&](int buf) {
#pragma unroll
            for (int k = 0; k < PRE; ++k)
                if (pk[k] >= 0) stage[buf * stage_f4 + (pk[k] >> 8) * stride + (pk[k] & 255)] = pre[k];
        };

        if (n_st > 0) { load_stage(t0); store_stage(0); }
        __syncthreads();
        for (int64_t s = 0; s < n_st; ++s) {
            const int64_t tile_first = t0 + s * TPS;
            if (s + 1 < n_st) load_stage(tile_first + TPS);
            if (active) {
                const float4* st = stage + (s & 1) * stage_f4;
                f32x4 acc[TPS];
                float ibv[TPS];
#pragma unroll
                for (int j = 0; j < TPS; ++j) { acc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; ibv[j] = 0.f; }
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    if (it < nit) {                                // uniform trip count; pieces past the row are zero
                        const int c = 4 * it + q;
                        const float4 a = ureg[it];
#pragma unroll
                        for (int j = 0; j < TPS; ++j) {
                            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (c < nch) b = st[(16 * j + r) * stride + c];
                            if (bias && c == 0) ibv[j] = b.x;      // (the user's column 0 is already zero in ureg)
                            acc[j] = WMF_MFMA16(a.x, b.x, acc[j]); acc[j] = WMF_MFMA16(a.y, b.y, acc[j]);
                            acc[j] = WMF_MFMA16(a.z, b.z, acc[j]); acc[j] = WMF_MFMA16(a.w, b.w, acc[j]);
                        }
                    }
                }
                // acc[j][reg] = score(user 4 q + reg, item 16 (tile_first + j) + r); the item biases sit in the q = 0 lanes
#pragma unroll
                for (int j = 0; j < TPS; ++j) {
                    if (tile_first + j < t1) {
                        const int64_t item = 16 * (tile_first + j) + r;
                        const float ibr = __shfl(ibv[j], r);
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            const float sc = acc[j][reg] + (bias ? ubr[reg] + ibr : 0.f);
                            const unsigned long long key = ((unsigned long long)rec_key(sc) << 32) | (unsigned long long)(~(uint32_t)item);
                            bool take = item < n_items && u0 + 4 * q + reg < n_users && key > thr[reg];
                            if (take && seen_lo[reg] < seen_hi[reg]) {
                                int64_t lo = seen_lo[reg], hi = seen_hi[reg];
                                while (lo < hi) {                  // first entry >= item
                                    const int64_t mid = (lo + hi) >> 1;
                                    if (seen_indices[mid] < (int32_t)item) lo = mid + 1; else hi = mid;
                                }
                                take = !(lo < seen_hi[reg] && seen_indices[lo] == (int32_t)item);
                            }
                            if (take) {
                                const int slot = atomicAdd(&cnt[4 * q + reg], 1);        // at most 16 per user and tile: below cap
                                if (slot < cap) keys[(4 * q + reg) * cap + slot] = key;
                            }
                        }
                        rec_wave_sync();
                        // a buffer the next tile could overflow is cut back to its topn best
                        const unsigned full = (unsigned)(__ballot(cnt[r] > cap - 16) & 0xFFFFull);
                        if (full) {
                            rec_compact(full, keys, cnt, thr_l, cap, topn, lane);
#pragma unroll
                            for (int reg = 0; reg < 4; ++reg) thr[reg] = thr_l[4 * q + reg];
                        }
                    }
                }
            }
            if (s + 1 < n_st) store_stage((int)((s + 1) & 1));
            __syncthreads();
        }

        if (active) {
            rec_compact((unsigned)(__ballot(cnt[r] > 0) & 0xFFFFull), keys, cnt, thr_l, cap, topn, lane);
            for (int u = 0; u < 16 && u0 + u < n_users; ++u) {
                unsigned long long* out = partial + ((u0 + u) * n_slices + sl) * topn;
                const int n = cnt[u];
                for (int k = lane; k < topn; k += 64) out[k] = k < n ? keys[u * cap + k] : 0ull;
            }
            rec_wave_sync();                                       // the buffers are read before the next pair resets them
        }
    }
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
            if (place < topn) {
                out_items[b * topn + place] = (int32_t)(~(uint32_t)(key & 0xFFFFFFFFull));
                if (out_scores) out_scores[b * topn + place] = rec_unkey((uint32_t)(key >> 32));
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
        const int count = min(mine, topn);
        for (int k = count + lane; k < topn; k += 64) {
            out_items[b * topn + k] = -1;
            if (out_scores) out_scores[b * topn + k] = -__builtin_inff();
        }
        if (lane == 0 && out_count) out_count[b] = count;
    }
}

// ---- launcher ---------------------------------------------------------------------------------------------------------------
static inline int rec_cap(int64_t topn) { return (int)(2 * topn > 32 ? 2 * topn : 32); }       // >= topn + 16, <= 256
static inline int rec_waves(int64_t topn) { return rec_cap(topn) <= 128 ? 4 : 2; }               // 64 KB of key buffers at most

int64_t wmf_recommend_ws_bytes(int64_t n_users, int64_t topn, int32_t n_slices) {
    if (n_users < 1 || topn < 1 || n_slices < 0) return 256;
    const int64_t s = n_slices == 0 ? WMF_RECOMMEND_AUTO_SLICES : n_slices;
    return WMF_RECOMMEND_WS_BASE + WMF_RECOMMEND_WS_PER_KEY * n_users * topn * s;
}

static int rec_cu_count() {
    static const int cus = [] {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
        return n;
    }();
    return cus;
}

// the slices of a call: as many as give every CU two workgroups, at least WMF_REC_SLICE_TILES tiles each, the cap at most
int wmf_recommend_slices(int64_t n_users, int64_t n_items, int64_t topn, int32_t n_slices) {
    if (n_slices > 0) return n_slices;
    const int64_t blocks = (n_users + 16 * rec_waves(topn) - 1) / (16 * rec_waves(topn));
    const int64_t tiles = (n_items + 15) / 16;
    int64_t s = (2 * (int64_t)rec_cu_count() + blocks - 1) / blocks;
    const int64_t by_tiles = (tiles + WMF_REC_SLICE_TILES - 1) / WMF_REC_SLICE_TILES;
    if (s > by_tiles) s = by_tiles;
    if (s > WMF_RECOMMEND_AUTO_SLICES) s = WMF_RECOMMEND_AUTO_SLICES;
    return (int)(s < 1 ? 1 : s);
}

template <int NIT, int TPS>
static int rec_launch_scan(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users,
                           int64_t n_items, const int64_t* seen_indptr, const int32_t* seen_indices, int topn, int n_slices,
                           unsigned long long* partial, hipStream_t st) {
    const int nw = rec_waves(topn), cap = rec_cap(topn), nch = ld >> 2;
    const size_t lds = (size_t)2 * TPS * 16 * (nch | 1) * 16 + ((size_t)nw * 16 * cap + nw * 16) * 8 + (size_t)nw * 16 * 4;
    const int64_t tiles = (n_items + 15) / 16, tiles_per_slice = (tiles + n_slices - 1) / n_slices;
    const int64_t n_work = ((n_users + 16 * nw - 1) / (16 * nw)) * n_slices;
    const int64_t grid = n_work < WMF_REC_SCAN_GRID ? n_work : WMF_REC_SCAN_GRID;
    static const char* name = wmf_kname("recommend_scan_kernel<%d, %d>", NIT, TPS);
    WMF_LAUNCH_LDS(name, (recommend_scan_kernel<NIT, TPS>), 112 * 1024, dim3((unsigned)grid), dim3(64 * nw), lds, st, users, items, ld, bias,
                   user_idx, n_users, n_items, seen_indptr, seen_indices, topn, cap, n_slices, tiles_per_slice, n_work, partial);
    return WMF_L_OK;
}

int wmf_launch_recommend(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users,
                         int64_t n_items, const int64_t* seen_indptr, const int32_t* seen_indices, int64_t topn, int32_t n_slices,
                         int32_t* out_items, float* out_scores, int32_t* out_count, void* ws, hipStream_t st) {
    const int slices = wmf_recommend_slices(n_users, n_items, topn, n_slices);
    unsigned long long* partial = reinterpret_cast<unsigned long long*>(ws);
    const int nit = ((ld >> 2) + 3) >> 2;
    int rc;
    if (nit <= 4) rc = rec_launch_scan<4, 4>(users, items, ld, bias, user_idx, n_users, n_items, seen_indptr, seen_indices, (int)topn, slices, partial, st);
    else if (nit <= 9) rc = rec_launch_scan<9, 2>(users, items, ld, bias, user_idx, n_users, n_items, seen_indptr, seen_indices, (int)topn, slices, partial, st);
    else if (nit <= 17) rc = rec_launch_scan<17, 1>(users, items, ld, bias, user_idx, n_users, n_items, seen_indptr, seen_indices, (int)topn, slices, partial, st);
    else return WMF_L_NO_KERNEL;
    if (rc) return rc;
    int64_t grid = (n_users + 3) / 4;
    if (grid > WMF_REC_MERGE_GRID) grid = WMF_REC_MERGE_GRID;
    WMF_LAUNCH("recommend_merge_kernel", recommend_merge_kernel, dim3((unsigned)grid), dim3(256), 0, st, partial, n_users, slices, (int)topn,
               out_items, out_scores, out_count);
    return WMF_L_OK;
}
