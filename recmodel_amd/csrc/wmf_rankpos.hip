// Exact full-catalogue ranks of held-out items (gfx950): for every target item of every row of a batch, the place it takes in
// wmf_recommend_topn's order of the row -- the number of unseen items of [0, n_items) whose key is strictly above the target's.
// The dual of wmf_recommend.hip: no selection, no key buffers, no merge of lists; the scoring loop with a counting epilogue.
//
//   * rankpos_target_kernel -- one wave per row: the scores of the row's first WMF_RANKPOS_MAX_TARGETS targets as the diagonal
//                              use of score_tile_kernel's operand pattern (wmf_rank.hip): the 16 A rows are 16 copies of the
//                              row's user, the B rows its targets, so the scores are bit-identical to the scan's.  The 64-bit
//                              keys (rec_key of the score, ~item: the order of wmf_recommend.hip) are sorted ascending into the
//                              workspace; targets past the limit get WMF_RANKPOS_BEYOND.
//   * rankpos_scan_kernel   -- the staging and operand layout of recommend_scan_kernel: 16 users per wave in registers, tiles
//                              of 16 items double-buffered in LDS, (user block, slice) work units.  A key at or below the user's
//                              lowest target key beats nothing (the early-out); one above the highest beats every target (a
//                              register counter); one in between is placed among the sorted target keys in LDS and counted in
//                              the bucket "beats exactly m targets" (an LDS integer atomic).  Seen items are NOT looked up here:
//                              every item of the catalogue is counted.  A unit ends with the suffix sums of its buckets added to
//                              the row's counters in the workspace by integer atomics.
//   * rankpos_finish_kernel -- one wave per row: the row's seen items scored by the same diagonal tile, one taken from every
//                              target whose key is below the seen item's; a target whose key EQUALS a seen item's is that
//                              item (same user, same item, same score) and gets WMF_RANKPOS_SEEN.  O(nnz_seen x targets).
// All accumulation is in integers, so the result cannot depend on the slices, the grid or the order of the atomics.

#include "wmf_common.h"
#include "wmf_internal.h"

#define WMF_RANKPOS_SCAN_GRID 4096   /* workgroups of the scan: (user block, slice) pairs beyond it take another trip */
#define WMF_RANKPOS_ROW_GRID 1024    /* workgroups of the two per-row kernels, four rows each */
#define RP_T WMF_RANKPOS_MAX_TARGETS
static_assert(RP_T == 16, "the per-row kernels hold a row's targets in the 16 rows of one MFMA tile");

int wmf_recommend_slices(int64_t n_users, int64_t n_items, int64_t topn, int32_t n_slices);   // wmf_recommend.hip

// rec_key of wmf_recommend.hip: ascending in the float order, -0.0 = +0.0
__device__ __forceinline__ uint32_t rp_score_key(float s) {
    uint32_t u = __builtin_bit_cast(uint32_t, s);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long rp_key(float s, int64_t item) {
    return ((unsigned long long)rp_score_key(s) << 32) | (unsigned long long)(~(uint32_t)item);
}
__device__ __forceinline__ unsigned long long rp_shfl64(unsigned long long v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ void rp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// score(user row, item row of lane r), valid in the lanes q == 0: score_tile_kernel's loop with the same user in all 16 A rows --
// lane (r, q) holds pieces 4 it + q, four MFMAs per piece in x, y, z, w order, column 0 zeroed and ub + ib added last
__device__ __forceinline__ float rp_diag_score(const float4* __restrict__ urow, const float4* __restrict__ irow, int nch, int bias, int q) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float ub = 0.f, ib = 0.f;
    for (int c = q; c < ((nch + 3) & ~3); c += 4) {              // uniform trip count; pieces past the row are zero
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (c < nch) { a = urow[c]; b = irow[c]; }
        if (bias && c == 0) { ub = a.x; ib = b.x; a.x = 0.f; }
        acc = WMF_MFMA16(a.x, b.x, acc); acc = WMF_MFMA16(a.y, b.y, acc);
        acc = WMF_MFMA16(a.z, b.z, acc); acc = WMF_MFMA16(a.w, b.w, acc);
    }
    return acc[0] + (bias ? ub + ib : 0.f);
}

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
        const float s = rp_diag_score(reinterpret_cast<const float4*>(users + (int64_t)user_idx[b] * ld),
                                      reinterpret_cast<const float4*>(items + item * ld), nch, bias, q);
        const unsigned long long key = (lane < nt) ? rp_key(s, item) : ~0ull;
        int pos = 0;                                               // the key's place among the 16 of lanes 0 .. 15, ascending
#pragma unroll
        for (int o = 0; o < RP_T; ++o) {
            const unsigned long long ko = rp_shfl64(key, o);
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

// NIT: trips of the feature loop a wave can hold a user row for (4 NIT pieces of 16 bytes per row); TPS: 16-item tiles per stage.
// Four waves.  Dynamic LDS: [two stages of TPS x 16 item rows, (nch | 1) pieces apart][sorted target keys: 16 users x RP_T per wave]
// [buckets: 16 users x (RP_T + 1) per wave].
template <int NIT, int TPS>
__global__ __launch_bounds__(256) void rankpos_scan_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld, int bias,
                                                           const int32_t* __restrict__ user_idx, int64_t n_rows, int64_t n_items,
                                                           const unsigned long long* __restrict__ tkey, const int32_t* __restrict__ tn,
                                                           int n_slices, int64_t tiles_per_slice, int64_t n_work,
                                                           unsigned int* __restrict__ counts) {
    extern __shared__ __align__(16) unsigned char rp_smem[];
    constexpr int PRE = (TPS * NIT + 3) / 4;                      // 16-byte pieces of a stage per thread, at 256 threads
    constexpr int NW = 4, HB = RP_T + 1;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2, nit = (nch + 3) >> 2, stride = nch | 1;
    const int stage_f4 = TPS * 16 * stride;
    float4* stage = reinterpret_cast<float4*>(rp_smem);
    unsigned long long* tk = reinterpret_cast<unsigned long long*>(rp_smem + (size_t)2 * stage_f4 * 16) + wave * 16 * RP_T;
    int* hist = reinterpret_cast<int*>(rp_smem + (size_t)2 * stage_f4 * 16 + (size_t)NW * 16 * RP_T * 8) + wave * 16 * HB;
    const float4* items4 = reinterpret_cast<const float4*>(items);
    const int64_t tiles = (n_items + 15) >> 4;

    // this thread's pieces of a stage: (item row of the stage) << 8 | piece
    int pk[PRE];
#pragma unroll
    for (int k = 0; k < PRE; ++k) {
        const int idx = tid + k * 256;
        pk[k] = idx < TPS * 16 * nch ? ((idx / nch) << 8) | (idx % nch) : -1;
    }

    for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        const int64_t ub = w / n_slices;
        const int sl = (int)(w % n_slices);
        const int64_t u0 = (ub * NW + wave) * 16;                  // first batch position of this wave
        const bool active = u0 < n_rows;
        const int64_t t0 = min((int64_t)sl * tiles_per_slice, tiles), t1 = min(t0 + tiles_per_slice, tiles);
        const int64_t n_st = (t1 - t0 + TPS - 1) / TPS;

        // the wave's 16 user rows, for the whole scan: lane (r, q) holds pieces 4 it + q of user r
        float4 ureg[NIT];
        float ubr[4] = {0.f, 0.f, 0.f, 0.f};
        {
            const float4* urow = reinterpret_cast<const float4*>(users + (int64_t)user_idx[min(u0 + r, n_rows - 1)] * ld);
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
        // the sorted target keys of the wave's users (a row past the batch has none) and empty buckets
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = lane + 64 * k;
            const int64_t b = u0 + (idx >> 4);
            tk[idx] = b < n_rows ? tkey[b * RP_T + (idx & 15)] : ~0ull;
        }
        for (int idx = lane; idx < 16 * HB; idx += 64) hist[idx] = 0;
        rp_wave_sync();
        unsigned long long tmin[4], tmax[4];
        int nt[4], all[4] = {0, 0, 0, 0};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t b = u0 + 4 * q + reg;
            nt[reg] = b < n_rows ? tn[b] : 0;
            tmin[reg] = tk[(4 * q + reg) * RP_T];                 // ~0 when the row has no targets: nothing passes
            tmax[reg] = tk[(4 * q + reg) * RP_T + max(nt[reg] - 1, 0)];
        }

        // the next stage on its way: plain unrolled loops that write every element (as lambdas with a skipped element the
        // array was kept in scratch)
        float4 pre[PRE];
#define RP_LOAD_STAGE(TILE_FIRST)                                                                                             \
    _Pragma("unroll") for (int k = 0; k < PRE; ++k) {                                                                         \
        const int64_t gi = min(16 * (TILE_FIRST) + (pk[k] >> 8), n_items - 1);   /* clamped: the scores are masked */          \
        pre[k] = pk[k] >= 0 ? items4[gi * nch + (pk[k] & 255)] : make_float4(0.f, 0.f, 0.f, 0.f);                              \
    }
#define RP_STORE_STAGE(BUF)                                                                                                   \
    _Pragma("unroll") for (int k = 0; k < PRE; ++k)                                                                           \
        if (pk[k] >= 0) stage[(BUF) * stage_f4 + (pk[k] >> 8) * stride + (pk[k] & 255)] = pre[k];

        if (n_st > 0) { RP_LOAD_STAGE(t0) RP_STORE_STAGE(0) }
        __syncthreads();
        for (int64_t s = 0; s < n_st; ++s) {
            const int64_t tile_first = t0 + s * TPS;
            if (s + 1 < n_st) { RP_LOAD_STAGE(tile_first + TPS) }
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
                            const unsigned long long key = rp_key(sc, item);
                            if (item < n_items && key > tmin[reg]) {
                                if (key > tmax[reg]) {
                                    ++all[reg];
                                } else {                           // tmin < key <= tmax: the targets strictly below it
                                    const unsigned long long* t = tk + (4 * q + reg) * RP_T;
                                    int m = 1;
                                    while (m < nt[reg] && t[m] < key) ++m;
                                    atomicAdd(&hist[(4 * q + reg) * HB + m], 1);
                                }
                            }
                        }
                    }
                }
            }
            if (s + 1 < n_st) { RP_STORE_STAGE((int)((s + 1) & 1)) }
            __syncthreads();
        }

        if (active) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg)
                if (all[reg]) atomicAdd(&hist[(4 * q + reg) * HB + nt[reg]], all[reg]);
            rp_wave_sync();
            // sorted slot i is beaten by every key that beats more than i targets
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = lane + 64 * k, u = idx >> 4, i = idx & 15;
                unsigned int c = 0;
                for (int m = i + 1; m <= RP_T; ++m) c += (unsigned int)hist[u * HB + m];
                if (c && u0 + u < n_rows) atomicAdd(&counts[(u0 + u) * RP_T + i], c);
            }
            rp_wave_sync();                                        // the buckets are read before the next pair resets them
        }
    }
}
#undef RP_LOAD_STAGE
#undef RP_STORE_STAGE

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
                const float s = rp_diag_score(urow, reinterpret_cast<const float4*>(items + id * ld), nch, bias, q);
                const unsigned long long sk = (valid && q == 0) ? rp_key(s, id) : 0ull;     // 0 is below every key
#pragma unroll
                for (int o = 0; o < 16; ++o) {
                    const unsigned long long ko = rp_shfl64(sk, o);
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

template <int NIT, int TPS>
static int rp_launch_scan(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_rows, int64_t n_items,
                          const RankposWs& w, int n_slices, hipStream_t st) {
    const int nch = ld >> 2;
    const size_t lds = (size_t)2 * TPS * 16 * (nch | 1) * 16 + (size_t)4 * 16 * RP_T * 8 + (size_t)4 * 16 * (RP_T + 1) * 4;
    const int64_t tiles = (n_items + 15) / 16, tiles_per_slice = (tiles + n_slices - 1) / n_slices;
    const int64_t n_work = ((n_rows + 63) / 64) * n_slices;
    const int64_t grid = n_work < WMF_RANKPOS_SCAN_GRID ? n_work : WMF_RANKPOS_SCAN_GRID;
    static const char* name = wmf_kname("rankpos_scan_kernel<%d, %d>", NIT, TPS);
    WMF_LAUNCH_LDS(name, (rankpos_scan_kernel<NIT, TPS>), 64 * 1024, dim3((unsigned)grid), dim3(256), lds, st, users, items, ld, bias, user_idx,
                   n_rows, n_items, w.tkey, w.tn, n_slices, tiles_per_slice, n_work, w.counts);
    return WMF_L_OK;
}

int wmf_launch_rank_positions(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_rows,
                              int64_t n_items, const int64_t* seen_indptr, const int32_t* seen_indices, const int64_t* target_indptr,
                              const int32_t* target_indices, int32_t n_slices, int32_t* out_rank, float* out_score, void* ws, hipStream_t st) {
    const int nit = ((ld >> 2) + 3) >> 2;
    if (nit > 17) return WMF_L_NO_KERNEL;
    const RankposWs w = rp_carve(ws, n_rows);
    const int slices = wmf_recommend_slices(n_rows, n_items, 1, n_slices);              // (topn = 1: the four-wave block of that scan)
    int64_t row_grid = (n_rows + 3) / 4;
    if (row_grid > WMF_RANKPOS_ROW_GRID) row_grid = WMF_RANKPOS_ROW_GRID;
    WMF_LAUNCH("rankpos_target_kernel", rankpos_target_kernel, dim3((unsigned)row_grid), dim3(256), 0, st, users, items, ld, bias, user_idx, n_rows,
               n_items, target_indptr, target_indices, out_rank, out_score, w.tkey, w.counts, w.tpos, w.tn);
    int rc;
    if (nit <= 4) rc = rp_launch_scan<4, 4>(users, items, ld, bias, user_idx, n_rows, n_items, w, slices, st);
    else if (nit <= 9) rc = rp_launch_scan<9, 2>(users, items, ld, bias, user_idx, n_rows, n_items, w, slices, st);
    else rc = rp_launch_scan<17, 1>(users, items, ld, bias, user_idx, n_rows, n_items, w, slices, st);
    if (rc) return rc;
    WMF_LAUNCH("rankpos_finish_kernel", rankpos_finish_kernel, dim3((unsigned)row_grid), dim3(256), 0, st, users, items, ld, bias, user_idx, n_rows,
               n_items, seen_indptr, seen_indices, target_indptr, w.tkey, w.counts, w.tpos, w.tn, out_rank);
    return WMF_L_OK;
}
