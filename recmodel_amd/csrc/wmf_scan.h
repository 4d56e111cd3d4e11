// What the serving kernels share (gfx950): the order-preserving score key, the 16 x 16 score tile of score_tile_kernel, and the
// full-catalogue scan of wmf_recommend.hip (a running top-n per user) and wmf_rankpos.hip (counts above the users' target keys):
// one scoring loop, the epilogue and the scoring rule as compile-time policies (wmf_similar.hip: the neighbours of a row).
#pragma once
#include "wmf_common.h"
#include "wmf_internal.h"

#define WMF_SCAN_GRID 4096           /* workgroups of a catalogue scan: (user block, slice) pairs beyond it take another trip */

// ---- score keys ---------------------------------------------------------------------------------------------------------------
// ascending in the float order (-0.0 below +0.0), of a float and of its bits
__device__ __forceinline__ uint32_t wmf_bits_key(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t wmf_float_key(float s) { return wmf_bits_key(__builtin_bit_cast(uint32_t, s)); }
// ... with -0.0 = +0.0: the key of the catalogue scans
__device__ __forceinline__ uint32_t wmf_score_key(float s) {
    const uint32_t u = __builtin_bit_cast(uint32_t, s);
    return wmf_bits_key(u == 0x80000000u ? 0u : u);
}
__device__ __forceinline__ float wmf_key_float(uint32_t k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}
// ONE total order of a user's items: a higher score wins, equal scores go to the lower id
__device__ __forceinline__ unsigned long long wmf_item_key(float s, int64_t item) {
    return ((unsigned long long)wmf_score_key(s) << 32) | (unsigned long long)(~(uint32_t)item);
}

// slot `at` of a top-n call's outputs: the item and the score of `key`, or the padding for 0 (no key of an item is 0: its low word is ~id)
__device__ __forceinline__ void rec_write_slot(int32_t* __restrict__ out_items, float* __restrict__ out_scores, int64_t at, unsigned long long key) {
    out_items[at] = key ? (int32_t)(~(uint32_t)(key & 0xFFFFFFFFull)) : -1;
    if (out_scores) out_scores[at] = key ? wmf_key_float((uint32_t)(key >> 32)) : -__builtin_inff();
}

__device__ __forceinline__ void wmf_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ unsigned long long wmf_shfl64(unsigned long long v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// ---- the score tile -------------------------------------------------------------------------------------------------------------
// 16 A rows x 16 B rows by f32 MFMA: lane (r, q) gives row r of each operand and reads pieces q, q + 4, ... of both, four MFMAs per
// piece in x, y, z, w order.  acc[reg] = sum over the columns of A row 4 q + reg times B row r; with bias, column 0 is left out of the
// sum and ub / ib hold column 0 of A row r / B row r in the lanes q == 0: the score is acc + ub + ib, added last.
struct WmfScoreTile { f32x4 acc; float ub, ib; };
__device__ __forceinline__ WmfScoreTile wmf_score_tile(const float4* arow, const float4* brow, int nch, int bias, int q) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    float ub = 0.f, ib = 0.f;
    for (int c = q; c < ((nch + 3) & ~3); c += 4) {              // uniform trip count; pieces past the row are zero
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (c < nch) { a = arow[c]; b = brow[c]; }
        if (bias && c == 0) { ub = a.x; ib = b.x; a.x = 0.f; }
        acc = WMF_MFMA16(a.x, b.x, acc); acc = WMF_MFMA16(a.y, b.y, acc);
        acc = WMF_MFMA16(a.z, b.z, acc); acc = WMF_MFMA16(a.w, b.w, acc);
    }
    return WmfScoreTile{acc, ub, ib};
}
// score(the one user of arow, item row of lane r), valid in the lanes q == 0: the tile with the same user in all 16 A rows
__device__ __forceinline__ float wmf_diag_score(const float4* __restrict__ urow, const float4* __restrict__ irow, int nch, int bias, int q) {
    const WmfScoreTile t = wmf_score_tile(urow, irow, nch, bias, q);
    return t.acc[0] + (bias ? t.ub + t.ib : 0.f);
}

// ---- the catalogue scan -----------------------------------------------------------------------------------------------------------
// Every score of rows x [0, n_items) in the arithmetic of the score tile (bit-identical), as 64-bit item keys handed to a policy.
// A workgroup of NW waves holds 16 rows per wave in registers and walks a contiguous SLICE of the catalogue's 16-item tiles, which
// it stages once in LDS for all its waves; the work units are the (block of 16 NW rows, slice) pairs.
// NIT: trips of the feature loop a wave can hold a row for (4 NIT pieces of 16 bytes per row); TPS: 16-item tiles per stage.
// Dynamic LDS: [two stages of TPS x 16 item rows, (nch | 1) pieces apart][the policy's][the scoring policy's, which its kernel
// places].  The policy P, a local of the kernel whose
// per-lane state is fixed-size arrays under compile-time indices, is called by every lane of a wave together:
//   p.begin(lds, u0, sl)                  a unit starts: lds = the dynamic LDS past the stages, u0 = the wave's first batch position
//                                         (waves past the batch are called too), sl = the slice
//   p.score(reg, j, item, key, in_range)  the key of (row u0 + 4 q + reg, item = 16 tile + r) of the stage's j-th tile; in_range:
//                                         the item exists (a row past the batch is a copy of the last one); with GATHER item is
//                                         the id of list position 16 tile + r, and the key is built from that id
//   p.tile(j)                             the four scores of the j-th tile are out
//   p.end()                               the slice is done; score, tile and end only in waves with u0 < n_rows
__host__ __device__ static inline size_t wmf_scan_stage_bytes(int tps, int ld) { return (size_t)2 * tps * 16 * ((ld >> 2) | 1) * 16; }

// What a score is made of besides the sum of the MFMAs is a second, compile-time policy S.  WmfModelScore (S::SCALED false) is the
// score of the model, wmf_score_tile's, as the text of the loop: acc + (user bias + item bias), the biases added last.  A policy with
// S::SCALED (wmf_similar.hip) leaves column 0 of a bias model out of both operands, adds nothing, and is called by every lane of a
// wave together (load and store by every thread of the workgroup):
//   s.rows(rs, user_idx, u0, n_rows, q)         rs[reg] = the per-row term of row u0 + 4 q + reg (the slot of the user bias)
//   s.load(tile_first, n_items) / s.store(buf)  with the global loads / the LDS stores of a stage: what travels with it
//   s.item(r, buf, j)                           the per-item term of item row r of the j-th tile of stage buffer buf
//   s.score(acc, rs, is)                        the score
struct WmfModelScore { static constexpr bool SCALED = false; };

// GATHER: the scan walks a LIST of catalogue rows instead of [0, n_items): n_items is the length of the list, position p stands for
// row cand_idx[p] (strictly ascending ids), and tiles and slices are cut from the positions.  The ids of a stage's 16 TPS positions
// travel with the stage like the scaled score's scales -- requested with its global loads, stored with its rows to cand_lds (two
// stages of TPS x 16 ids, which the kernel places) -- so the key and the policy get the real id from LDS.
template <int NIT, int TPS, int NW, class P, class S = WmfModelScore, bool GATHER = false>
__device__ __forceinline__ void wmf_catalogue_scan(const float* __restrict__ users, const float* __restrict__ items, int ld, int bias,
                                                   const int32_t* __restrict__ user_idx, int64_t n_rows, int64_t n_items, int n_slices,
                                                   int64_t tiles_per_slice, int64_t n_work, P& p, S sp = S(),
                                                   const int32_t* __restrict__ cand_idx = nullptr, int32_t* cand_lds = nullptr) {
    static_assert(!GATHER || TPS * 16 <= 64 * NW, "one thread per candidate id of a stage");
    extern __shared__ __align__(16) unsigned char wmf_scan_smem[];
    constexpr int PRE = (TPS * NIT + NW - 1) / NW;                // 16-byte pieces of a stage per thread
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2, nit = (nch + 3) >> 2, stride = nch | 1;
    const int stage_f4 = TPS * 16 * stride;
    float4* stage = reinterpret_cast<float4*>(wmf_scan_smem);
    const float4* items4 = reinterpret_cast<const float4*>(items);
    const int64_t tiles = (n_items + 15) >> 4;

    // this thread's pieces of a stage: (item row of the stage) << 8 | piece
    int pk[PRE];
#pragma unroll
    for (int k = 0; k < PRE; ++k) {
        const int idx = tid + k * 64 * NW;
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
            if constexpr (S::SCALED) {
                sp.rows(ubr, user_idx, u0, n_rows, q);
            } else {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) ubr[reg] = __shfl(ubv, 4 * q + reg);    // user bias of user 4 q + reg
            }
        }
        p.begin(wmf_scan_smem + wmf_scan_stage_bytes(TPS, ld), u0, sl);

        // the next stage on its way: plain unrolled loops that write every element (as lambdas with a skipped element the
        // array was kept in scratch)
        float4 pre[PRE];
        int32_t cand_pre = 0;                                      // (GATHER) this thread's id of the stage on its way (threads < 16 TPS)
#define WMF_SCAN_LOAD_STAGE(TILE_FIRST)                                                                                       \
    {                                                                                                                         \
        _Pragma("unroll") for (int k = 0; k < PRE; ++k) {                                                                     \
            int64_t gi = min(16 * (TILE_FIRST) + (pk[k] >> 8), n_items - 1);         /* clamped: the scores are masked */      \
            if constexpr (GATHER) gi = pk[k] >= 0 ? cand_idx[gi] : 0;                                                         \
            pre[k] = pk[k] >= 0 ? items4[gi * nch + (pk[k] & 255)] : make_float4(0.f, 0.f, 0.f, 0.f);                          \
        }                                                                                                                     \
        if constexpr (S::SCALED) sp.load(TILE_FIRST, n_items);                                                                \
        if constexpr (GATHER) {                                                                                               \
            if (tid < TPS * 16) cand_pre = cand_idx[min(16 * (TILE_FIRST) + (int64_t)tid, n_items - 1)];                      \
        }                                                                                                                     \
    }
#define WMF_SCAN_STORE_STAGE(BUF)                                                                                             \
    {                                                                                                                         \
        _Pragma("unroll") for (int k = 0; k < PRE; ++k)                                                                       \
            if (pk[k] >= 0) stage[(BUF) * stage_f4 + (pk[k] >> 8) * stride + (pk[k] & 255)] = pre[k];                         \
        if constexpr (S::SCALED) sp.store(BUF);                                                                               \
        if constexpr (GATHER) {                                                                                               \
            if (tid < TPS * 16) cand_lds[(BUF) * TPS * 16 + tid] = cand_pre;                                                  \
        }                                                                                                                     \
    }

        if (n_st > 0) { WMF_SCAN_LOAD_STAGE(t0) WMF_SCAN_STORE_STAGE(0) }
        __syncthreads();
        for (int64_t s = 0; s < n_st; ++s) {
            const int64_t tile_first = t0 + s * TPS;
            if (s + 1 < n_st) { WMF_SCAN_LOAD_STAGE(tile_first + TPS) }
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
                            if constexpr (S::SCALED) {
                                if (bias && c == 0) b.x = 0.f;     // the bias column is no feature
                            } else {
                                if (bias && c == 0) ibv[j] = b.x;  // (the user's column 0 is already zero in ureg)
                            }
                            acc[j] = WMF_MFMA16(a.x, b.x, acc[j]); acc[j] = WMF_MFMA16(a.y, b.y, acc[j]);
                            acc[j] = WMF_MFMA16(a.z, b.z, acc[j]); acc[j] = WMF_MFMA16(a.w, b.w, acc[j]);
                        }
                    }
                }
                // acc[j][reg] = score(user 4 q + reg, item 16 (tile_first + j) + r); the item biases sit in the q = 0 lanes
#pragma unroll
                for (int j = 0; j < TPS; ++j) {
                    if (tile_first + j < t1) {
                        const int64_t pos = 16 * (tile_first + j) + r;
                        int64_t item = pos;
                        if constexpr (GATHER) item = cand_lds[(int)(s & 1) * TPS * 16 + 16 * j + r];
                        float ibr;
                        if constexpr (S::SCALED) ibr = sp.item(r, (int)(s & 1), j); else ibr = __shfl(ibv[j], r);
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) {
                            float sc;
                            if constexpr (S::SCALED) sc = sp.score(acc[j][reg], ubr[reg], ibr); else sc = acc[j][reg] + (bias ? ubr[reg] + ibr : 0.f);
                            p.score(reg, j, item, wmf_item_key(sc, item), pos < n_items);
                        }
                        p.tile(j);
                    }
                }
            }
            if (s + 1 < n_st) { WMF_SCAN_STORE_STAGE((int)((s + 1) & 1)) }
            __syncthreads();
        }
        if (active) p.end();
    }
#undef WMF_SCAN_LOAD_STAGE
#undef WMF_SCAN_STORE_STAGE
}

// ---- the host side of a scan launch ---------------------------------------------------------------------------------------------
// What every launch of a catalogue scan takes, in the spirit of RowArgs.  Host only: a launch site unpacks it into the kernel's
// positional arguments.  tiles_per_slice, n_work and grid are wmf_scan_geometry's.
struct WmfScanArgs {
    const float* users; const float* items; int ld, bias; const int32_t* user_idx;
    int64_t n_rows, n_items; int n_slices; hipStream_t st;
    int64_t tiles_per_slice, n_work, grid;
};
// n_slices slices of the catalogue's 16-item tiles, one work unit per (block of 16 nw rows, slice), WMF_SCAN_GRID workgroups at most
static inline void wmf_scan_geometry(WmfScanArgs& a, int nw) {
    const int64_t tiles = (a.n_items + 15) / 16;
    a.tiles_per_slice = (tiles + a.n_slices - 1) / a.n_slices;
    a.n_work = ((a.n_rows + 16 * nw - 1) / (16 * nw)) * a.n_slices;
    a.grid = a.n_work < WMF_SCAN_GRID ? a.n_work : WMF_SCAN_GRID;
}
// The width class of a scan (as wmf_dispatch_list): fn(wmf_int<NIT>{}, wmf_int<TPS>{}) for the class that holds a row of ld floats,
// WMF_L_NO_KERNEL beyond the widest.  Exactly these three are instantiated.
template <class Fn>
static inline int wmf_dispatch_scan(int ld, Fn&& fn) {
    const int nit = ((ld >> 2) + 3) >> 2;
    if (nit <= 4) return fn(wmf_int<4>{}, wmf_int<4>{});
    if (nit <= 9) return fn(wmf_int<9>{}, wmf_int<2>{});
    if (nit <= 17) return fn(wmf_int<17>{}, wmf_int<1>{});
    return WMF_L_NO_KERNEL;
}
