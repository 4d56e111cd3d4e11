// Sampled top-n and the log-partition of the catalogue softmax (gfx950): wmf_sample_topn, wmf_log_partition, wmf_sample_noise.
//
// The n largest of z_i = score_i + T g_i, g_i i.i.d. standard Gumbel, are a Plackett-Luce sample without replacement from
// softmax(score / T) over the eligible items (the Gumbel-top-n identity), so a sampled list is ONE catalogue scan: nothing of size
// rows x items exists anywhere.  The noise is a pure function of (seed, stream, item) (wmf_noise.h); everything else is the wide
// top-n's (wmf_topn_wide.h): the scan, the width classes, the three filter forms, the workspace buffers and their exact cut.
//
//   * sample_scan_kernel    -- the catalogue scan with RecSampleWide, which IS RecTopNWide but for the key: it is rebuilt from
//                              z = fmaf(T, g, score) BEFORE the threshold test and the eligibility search.  The row's hash prefix
//                              is computed once per unit; an item whose fmaf(T, WMF_SAMPLE_G_MAX, score) cannot beat the row's
//                              threshold is dropped before its hash and its two logarithms (rounding is monotone and g <=
//                              WMF_SAMPLE_G_MAX, so the test is exact: the bits are those of the scan without it).  In the list
//                              form the noise is keyed by the real id.  T = 0: z = score, the keys and so the result of
//                              wmf_recommend_topn_wide, bit for bit.
//   * sample_select_kernel  -- rec_wide_select_row by the perturbed key, then the picks scored again in the score tile's
//                              arithmetic (wmf_diag_score: bit-identical to the scan) for out_scores; out_keys holds z.
//   * logz_scan_kernel      -- the same scan with RecLogPartition: every ELIGIBLE score (there is no threshold: the filter is asked
//                              for each) enters a running (max, sum) per lane and row, the max in float32, a term expf((s - m) / T)
//                              in float32, the sum in float64; a lane's partial of a (row, slice) goes to the workspace.
//   * logz_merge_kernel     -- one wave per row: the 16 n_slices partials combined in a fixed order in float64, written as float32.
// No float atomics anywhere: two runs at one slice count give the same bits; other slice counts differ by float64 rounding of the
// merge and by where a lane's running max was raised.
//   * sample_noise_kernel   -- g and k of arbitrary (stream, item) pairs from wmf_noise.h: what the exact tests stand on.

#include "wmf_common.h"
#include "wmf_internal.h"
#include "wmf_scan.h"
#include "wmf_topn_wide.h"
#include "wmf_noise.h"

#define WMF_SAMPLE_SELECT_GRID 1024  /* workgroups of the selection, one row each; rows beyond it take another trip */
#define WMF_LOGZ_MERGE_GRID 1024     /* workgroups of the log-partition merge, four rows each */
#define WMF_SAMPLE_NOISE_GRID 1024   /* workgroups of sample_noise_kernel */

// ---- the perturbing epilogue ------------------------------------------------------------------------------------------------
// RecTopNWide with the key of z in place of the key of the score.  a[reg]: the hash prefix of row u0 + 4 q + reg.
template <int NW, bool MASK>
struct RecSampleWide {
    RecTopNWide<NW, MASK> base;
    float temperature; uint64_t seed; const uint64_t* __restrict__ row_stream;
    uint64_t a[4];

    __device__ __forceinline__ void begin(unsigned char* lds, int64_t u0, int sl) {
        base.begin(lds, u0, sl);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t b = u0 + 4 * base.q + reg;
            a[reg] = wmf_noise_row(seed, (row_stream && b < base.n_users) ? row_stream[b] : (uint64_t)b);
        }
    }
    __device__ __forceinline__ void score(int reg, int j, int64_t item, unsigned long long key, bool in_range) {
        if (!in_range || base.u0 + 4 * base.q + reg >= base.n_users) return;
        const float s = wmf_key_float((uint32_t)(key >> 32));
        // no draw lifts this item over the row's threshold: z <= fmaf(T, G_MAX, s), and the key is monotone in z
        if (wmf_item_key(__builtin_fmaf(temperature, WMF_SAMPLE_G_MAX, s), item) <= base.thr[reg]) return;
        const float z = __builtin_fmaf(temperature, wmf_noise_g(wmf_noise_k(a[reg], (int32_t)item)), s);
        base.score(reg, j, item, wmf_item_key(z, item), true);
    }
    __device__ __forceinline__ void tile(int j) { base.tile(j); }
    __device__ __forceinline__ void end() { base.end(); }
};

template <int NIT, int TPS, int NW, int FORM>
__global__ __launch_bounds__(64 * NW) void sample_scan_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld, int bias,
                                                              const int32_t* __restrict__ user_idx, int64_t n_users, int64_t n_items,
                                                              WMF_FILTER_PARAMS, int topn, int cap, int n_slices, int64_t tiles_per_slice,
                                                              int64_t n_work, float temperature, uint64_t seed,
                                                              const uint64_t* __restrict__ row_stream, unsigned long long* keys_ws,
                                                              int32_t* counts_ws) {
    extern __shared__ __align__(16) unsigned char wmf_scan_smem[];
    RecSampleWide<NW, FORM == 1> p{{WMF_FILTER_FROM_PARAMS, n_users, topn, cap, n_slices, keys_ws, counts_ws}, temperature, seed, row_stream};
    wmf_catalogue_scan<NIT, TPS, NW, decltype(p), WmfModelScore, FORM == 2>(
        users, items, ld, bias, user_idx, n_users, n_items, n_slices, tiles_per_slice, n_work, p, WmfModelScore(), cand_idx,
        reinterpret_cast<int32_t*>(wmf_scan_smem + wmf_scan_stage_bytes(TPS, ld) + rec_wide_lds_bytes(NW)));
}

// One workgroup per batch position: the topn best perturbed keys of the row's slices, sorted best first (rec_wide_select_row): items,
// out_keys = z, count and padding from the keys; then out_scores, 16 picks per wave and trip: the model's score of each pick in the
// score tile's arithmetic, with -0.0 written as +0.0 as a key's score is.
__global__ __launch_bounds__(256) void sample_select_kernel(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ counts,
                                                            int64_t n_users, int n_slices, int topn, int cap, const float* __restrict__ users,
                                                            const float* __restrict__ items, int ld, int bias,
                                                            const int32_t* __restrict__ user_idx, int32_t* __restrict__ out_items,
                                                            float* __restrict__ out_scores, float* __restrict__ out_keys,
                                                            int32_t* __restrict__ out_count) {
    __shared__ unsigned long long sel[WMF_RECOMMEND_WIDE_MAX_TOPN];
    __shared__ unsigned hist[256];
    __shared__ int counters[2];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2;
    for (int64_t b = blockIdx.x; b < n_users; b += gridDim.x) {
        const int count = rec_wide_select_row(keys + (size_t)b * n_slices * cap, counts + b * n_slices, n_slices, topn, cap, sel, hist, counters, t);
        for (int k = t; k < topn; k += 256) rec_write_slot(out_items, out_keys, b * topn + k, k < count ? sel[k] : 0ull);
        if (out_scores) {
            const float4* urow = reinterpret_cast<const float4*>(users + (int64_t)user_idx[b] * ld);
            for (int k0 = 16 * wave; k0 < topn; k0 += 64) {        // (uniform in a wave: the score tile is an MFMA)
                const int k = k0 + r;
                float sc = -__builtin_inff();
                if (k0 < count) {
                    const int64_t item = (int64_t)(~(uint32_t)(sel[min(k, count - 1)] & 0xFFFFFFFFull));
                    sc = wmf_diag_score(urow, reinterpret_cast<const float4*>(items + item * ld), nch, bias, q);
                    sc = wmf_key_float(wmf_score_key(sc));
                }
                if (q == 0 && k < topn) out_scores[b * topn + k] = k < count ? sc : -__builtin_inff();
            }
        }
        if (t == 0 && out_count) out_count[b] = count;
        __syncthreads();                                           // sel and the counters are read before the next row resets them
    }
}

// ---- the log-partition epilogue ---------------------------------------------------------------------------------------------
// What a lane knows of a (row, slice) pair when the slice is done: the largest eligible score it saw, the sum of expf((s - m) / T)
// over its eligible scores, and their number.  Workspace: partial[((b * n_slices + slice) * 16) + r], r the lane's item column.
struct WmfLogzPartial { double sum; float m; int32_t cnt; };
static_assert(sizeof(WmfLogzPartial) == WMF_LOG_PARTITION_WS_PER_LANE, "the workspace formula of include/wmf_hip.h");

template <int NW, bool MASK>
struct RecLogPartition {
    WmfRowFilter filter;
    int64_t n_users; int n_slices; float temperature; WmfLogzPartial* __restrict__ partial_ws;
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    int64_t u0; int sl;
    float m[4]; double sum[4]; int cnt[4];
    WmfRowEligible<false, MASK> ok;

    __device__ __forceinline__ void begin(unsigned char*, int64_t u0_, int sl_) {
        u0 = u0_; sl = sl_;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) { m[reg] = -__builtin_inff(); sum[reg] = 0.0; cnt[reg] = 0; }
        ok.begin(filter, u0, q, n_users);
    }
    __device__ __forceinline__ void score(int reg, int, int64_t item, unsigned long long key, bool in_range) {
        if (in_range && u0 + 4 * q + reg < n_users && ok.pass(reg, item)) {
            ++cnt[reg];
            const float s = wmf_key_float((uint32_t)(key >> 32));
            if (s > m[reg]) {                                      // the sum so far in units of the new max (the first score: 0 * 0 + 1)
                sum[reg] = sum[reg] * (double)expf((m[reg] - s) / temperature) + 1.0;
                m[reg] = s;
            } else if (s > -__builtin_inff()) {                    // (a score of -inf weighs nothing; s == m: also for m = +inf)
                sum[reg] += (double)(s == m[reg] ? 1.f : expf((s - m[reg]) / temperature));
            }
        }
    }
    __device__ __forceinline__ void tile(int) {}
    __device__ __forceinline__ void end() {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t b = u0 + 4 * q + reg;
            if (b < n_users) partial_ws[((size_t)b * n_slices + sl) * 16 + r] = WmfLogzPartial{sum[reg], m[reg], cnt[reg]};
        }
    }
};

template <int NIT, int TPS, int NW, int FORM>
__global__ __launch_bounds__(64 * NW) void logz_scan_kernel(const float* __restrict__ users, const float* __restrict__ items, int ld, int bias,
                                                            const int32_t* __restrict__ user_idx, int64_t n_users, int64_t n_items,
                                                            WMF_FILTER_PARAMS, int n_slices, int64_t tiles_per_slice, int64_t n_work,
                                                            float temperature, WmfLogzPartial* __restrict__ partial_ws) {
    extern __shared__ __align__(16) unsigned char wmf_scan_smem[];
    RecLogPartition<NW, FORM == 1> p{WMF_FILTER_FROM_PARAMS, n_users, n_slices, temperature, partial_ws};
    wmf_catalogue_scan<NIT, TPS, NW, decltype(p), WmfModelScore, FORM == 2>(
        users, items, ld, bias, user_idx, n_users, n_items, n_slices, tiles_per_slice, n_work, p, WmfModelScore(), cand_idx,
        reinterpret_cast<int32_t*>(wmf_scan_smem + wmf_scan_stage_bytes(TPS, ld)));
}

// One wave per row: M = the largest max of the row's 16 n_slices partials, S = sum of sum_e exp((m_e - M) / T) in float64 -- lane l
// adds the partials l, l + 64, ... in that order, then a butterfly over the lanes (a + b is b + a: every lane holds the same bits) --
// log Z = M / T + log S, rounded to float32 once.  Nothing eligible, or nothing above -inf: -inf.
__global__ __launch_bounds__(256) void logz_merge_kernel(const WmfLogzPartial* __restrict__ partial, int64_t n_rows, int n_slices, float temperature,
                                                         float* __restrict__ out_logz, int32_t* __restrict__ out_eligible) {
    const int lane = threadIdx.x & 63;
    const int n = n_slices * 16;
    for (int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); b < n_rows; b += (int64_t)gridDim.x * 4) {
        const WmfLogzPartial* P = partial + (size_t)b * n;
        float M = -__builtin_inff();
        int c = 0;
        for (int e = lane; e < n; e += 64) { M = fmaxf(M, P[e].m); c += P[e].cnt; }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { M = fmaxf(M, __shfl_xor(M, o)); c += __shfl_xor(c, o); }
        double S = 0.0;
        for (int e = lane; e < n; e += 64) {
            const WmfLogzPartial pe = P[e];
            if (pe.sum > 0.0) S += pe.m == M ? pe.sum : pe.sum * exp(((double)pe.m - (double)M) / (double)temperature);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) S += __shfl_xor(S, o);
        if (lane == 0) {
            out_logz[b] = (S > 0.0) ? (float)((double)M / (double)temperature + log(S)) : -__builtin_inff();
            if (out_eligible) out_eligible[b] = c;
        }
    }
}

// ---- the noise of arbitrary pairs ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_noise_kernel(uint64_t seed, const uint64_t* __restrict__ row_stream, const int32_t* __restrict__ items,
                                                           int64_t n_pairs, float* __restrict__ out_g, uint32_t* __restrict__ out_k) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += (int64_t)gridDim.x * 256) {
        const uint32_t k = wmf_noise_k(wmf_noise_row(seed, row_stream ? row_stream[i] : (uint64_t)i), items[i]);
        if (out_k) out_k[i] = k;
        if (out_g) out_g[i] = wmf_noise_g(k);
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
// the workspace and the slices of wmf_recommend_topn_wide: [keys: n_users x n_slices buffers of cap][counts: one per buffer]
int wmf_launch_sample(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users, int64_t n_items,
                      const WmfRowFilter& flt, int64_t n_cand, int64_t topn, int32_t n_slices, float temperature, uint64_t seed,
                      const uint64_t* row_stream, int32_t* out_items, float* out_scores, float* out_keys, int32_t* out_count, void* ws,
                      hipStream_t st) {
    const int64_t n_scan = flt.cand_idx ? n_cand : n_items;
    WmfScanArgs a = {users, items, ld, bias, user_idx, n_users, n_scan, wmf_recommend_wide_slices(n_users, n_scan, topn, n_slices), st};
    constexpr int NW = WMF_REC_WIDE_WAVES;
    wmf_scan_geometry(a, NW);
    const int cap = WMF_RECOMMEND_WIDE_CAP(topn);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws);
    int32_t* counts = reinterpret_cast<int32_t*>(keys + (size_t)n_users * a.n_slices * cap);
    const int rc = wmf_dispatch_scan(ld, [&](auto nit, auto tps) {
        return wmf_dispatch_list<0, 1, 2>(rec_form(flt), [&](auto form) {
            constexpr int NIT = decltype(nit)::value, TPS = decltype(tps)::value, FORM = decltype(form)::value;
            static const char* name = wmf_kname("sample_scan_%skernel<%d, %d, %d>", REC_FORM_NAME[FORM], NIT, TPS, NW);
            WMF_LAUNCH_LDS(name, (sample_scan_kernel<NIT, TPS, NW, FORM>), 112 * 1024, dim3((unsigned)a.grid), dim3(64 * NW),
                           wmf_scan_stage_bytes(TPS, ld) + rec_wide_lds_bytes(NW) + rec_form_lds(TPS, FORM), st, a.users, a.items, a.ld,
                           a.bias, a.user_idx, a.n_rows, a.n_items, WMF_FILTER_ARGS(flt), (int)topn, cap, a.n_slices, a.tiles_per_slice, a.n_work,
                           temperature, seed, row_stream, keys, counts);
            return (int)WMF_L_OK;
        });
    });
    if (rc) return rc;
    const int64_t grid = n_users < WMF_SAMPLE_SELECT_GRID ? n_users : WMF_SAMPLE_SELECT_GRID;
    WMF_LAUNCH("sample_select_kernel", sample_select_kernel, dim3((unsigned)grid), dim3(256), 0, st, keys, counts, n_users, a.n_slices, (int)topn, cap,
               users, items, ld, bias, user_idx, out_items, out_scores, out_keys, out_count);
    return WMF_L_OK;
}

int64_t wmf_log_partition_ws_bytes(int64_t n_rows, int32_t n_slices) {
    if (n_rows < 1 || n_slices < 0) return WMF_RECOMMEND_WIDE_WS_BASE;
    return WMF_RECOMMEND_WIDE_WS_BASE + wmf_recommend_wide_lists(n_rows, n_slices) * 16 * WMF_LOG_PARTITION_WS_PER_LANE;
}

// the slices of wmf_recommend_topn_wide at topn 1: the lists of the workspace, a slice of 1024 positions at least
int wmf_launch_log_partition(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_rows, int64_t n_items,
                             const WmfRowFilter& flt, int64_t n_cand, float temperature, int32_t n_slices, float* out_logz,
                             int32_t* out_eligible, void* ws, hipStream_t st) {
    const int64_t n_scan = flt.cand_idx ? n_cand : n_items;
    WmfScanArgs a = {users, items, ld, bias, user_idx, n_rows, n_scan, wmf_recommend_wide_slices(n_rows, n_scan, 1, n_slices), st};
    constexpr int NW = WMF_REC_WIDE_WAVES;
    wmf_scan_geometry(a, NW);
    WmfLogzPartial* partial = reinterpret_cast<WmfLogzPartial*>(ws);
    const int rc = wmf_dispatch_scan(ld, [&](auto nit, auto tps) {
        return wmf_dispatch_list<0, 1, 2>(rec_form(flt), [&](auto form) {
            constexpr int NIT = decltype(nit)::value, TPS = decltype(tps)::value, FORM = decltype(form)::value;
            static const char* name = wmf_kname("logz_scan_%skernel<%d, %d, %d>", REC_FORM_NAME[FORM], NIT, TPS, NW);
            WMF_LAUNCH_LDS(name, (logz_scan_kernel<NIT, TPS, NW, FORM>), 112 * 1024, dim3((unsigned)a.grid), dim3(64 * NW),
                           wmf_scan_stage_bytes(TPS, ld) + rec_form_lds(TPS, FORM), st, a.users, a.items, a.ld, a.bias, a.user_idx, a.n_rows,
                           a.n_items, WMF_FILTER_ARGS(flt), a.n_slices, a.tiles_per_slice, a.n_work, temperature, partial);
            return (int)WMF_L_OK;
        });
    });
    if (rc) return rc;
    int64_t grid = (n_rows + 3) / 4;
    if (grid > WMF_LOGZ_MERGE_GRID) grid = WMF_LOGZ_MERGE_GRID;
    WMF_LAUNCH("logz_merge_kernel", logz_merge_kernel, dim3((unsigned)grid), dim3(256), 0, st, partial, n_rows, a.n_slices, temperature, out_logz,
               out_eligible);
    return WMF_L_OK;
}

void wmf_launch_sample_noise(uint64_t seed, const uint64_t* row_stream, const int32_t* items, int64_t n_pairs, float* out_g, uint32_t* out_k,
                             hipStream_t st) {
    int64_t grid = (n_pairs + 255) / 256;
    if (grid > WMF_SAMPLE_NOISE_GRID) grid = WMF_SAMPLE_NOISE_GRID;
    WMF_LAUNCH("sample_noise_kernel", sample_noise_kernel, dim3((unsigned)grid), dim3(256), 0, st, seed, row_stream, items, n_pairs, out_g, out_k);
}
