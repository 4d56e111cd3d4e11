// Internal launcher declarations shared by the .hip translation units of libwmf_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "../../include/wmf_hip.h"
#include "wmf_filter.h"

#define WMF_GRAM_MAX_WAVES 4096
#define WMF_EVAL_MAX_BLOCKS 2048
#define WMF_AUDIT_MAX_BLOCKS 2048
#define WMF_HEAVY_T 4096      /* rows with more stored entries are accumulated by several waves ... */
#define WMF_SEG 2048          /* ... in segments of this many entries */
#define WMF_WIDE_LU_GRID 64   /* workgroups (and workspace slices) of the pivoted-LU fallback for f > 144 */

// The kernel-selection switches (include/wmf_hip.h, WMF_DBG_*); 0 in normal use.  The shipped library accepts the switches a
// committed GPU test sets; a lab build (-DWMF_LAB, `make lab`) accepts every one, and only it compiles the kernels that the
// other switches select: their launch sites sit behind `if constexpr (WMF_LAB_BUILD)`.
extern int wmf_debug_flags;
#ifdef WMF_LAB
constexpr bool WMF_LAB_BUILD = true;
#else
constexpr bool WMF_LAB_BUILD = false;
#endif
constexpr int WMF_DBG_SHIPPED = WMF_DBG_HEAVY_REG_RING | WMF_DBG_F32_GRAM | WMF_DBG_HEAVY_ONE_WAVE | WMF_DBG_F64_NO_LOW_RANK |
                                WMF_DBG_NO_ITER | WMF_DBG_F64_VALU;
constexpr int WMF_DBG_LAB = WMF_DBG_NO_ELIMINATION | WMF_DBG_NO_ACCUMULATION | WMF_DBG_NO_TILE_INVERSE | WMF_DBG_LOW32_GAUSS_JORDAN |
                            WMF_DBG_NO_BORDER | WMF_DBG_WIDE_EIGHT_WAVES | WMF_DBG_NO_ROW_PAIRS | WMF_DBG_HEAVY_F32_ACC |
                            WMF_DBG_HEAVY_REG_RING_K64 | WMF_DBG_F32_TRANSFORM | WMF_DBG_LOW_F32_TILES | WMF_DBG_WIDE_F32 |
                            WMF_DBG_HEAVY_PIVOTED_LU | WMF_DBG_F64_TEAMS | WMF_DBG_NO_ROLLED_LAYOUT;
constexpr int WMF_DBG_ACCEPTED = WMF_LAB_BUILD ? (WMF_DBG_SHIPPED | WMF_DBG_LAB) : WMF_DBG_SHIPPED;   // what wmf_debug_set_flags takes

// row-degree bins of a plan
enum { WMF_BIN_LOW16 = 0, WMF_BIN_LOW32 = 1, WMF_BIN_MFMA = 2, WMF_BIN_GENERAL = 3, WMF_NBINS = 4 };

struct wmf_plan {
    int64_t n;                 // rows
    int f;
    int64_t count[WMF_NBINS];  // rows per bin
    int64_t count8, nnz8;      // rows of the first bin with at most 8 entries (and their entries); they come first in rows[WMF_BIN_LOW16]
    bool bias;                 // created for a biased model: w_eff is allocated (unless split)
    bool split;                // latched at creation: the whitened fixed side comes in the split layout (no w_eff needed)
    int64_t nnz[WMF_NBINS];    // stored entries per bin
    int32_t* rows[WMF_NBINS];  // device: row ids of each bin (slices of rows_all)
    int32_t* rows_all;         // device: n row ids grouped by bin
    int32_t* fallback_rows;    // device: n slots, rows bounced to the general kernel at run time
    int32_t* fallback_count;   // device: 1 counter
    float* w_eff;              // device: nnz effective weights (values - bias[indices]) of a biased model
    // rows of the MFMA bin with more than WMF_HEAVY_T entries sit at the end of that bin and are split into segments
    int64_t heavy_count, heavy_nnz, seg_total;
    int64_t* seg_lo;           // device: first entry of each segment
    int32_t* seg_d;            // device: entries in each segment
    int32_t* seg_first;        // device: heavy_count + 1 prefix of segment counts
    float* partial;            // device: seg_total x (tiles x 256) partial accumulators
    float* wide_ws;            // device: workspace of the f > 144 pivoted-LU fallback
    // round 4: the first iter_count rows of the heavy bin's ordinary rows have at most wmf_iter_dmax entries: candidates of the
    // matrix-free iteration kernel (wmf_iter.hip); fallback_count[1] counts the rows it hands back in iter_bounce_rows
    int64_t iter_count, iter_nnz;
    int iter_dmax;             // the candidates' longest admissible row at the width / layout the plan was created for
    int32_t* iter_bounce_rows; // device: 2 x iter_count slots (the rows handed back to the elimination kernels | stage 1's hand-on list)
    int32_t* iter_info;        // device: iter_count x {first entry (low, high word), row id, entries}: a candidate's bookkeeping in one 16-byte load
    unsigned long long* iter_stats;   // device: 8 counters (4 reported), accumulated over the launches (wmf_plan_iter_stats reads and clears)
};

int wmf_gram_max_waves(int f);
int wmf_gram_nwaves(int64_t m, int f);
int wmf_launch_gram(const float* Y, int64_t m, int f, int ld, int bias, double* G_sum, float* partial, double* slices,
                    hipStream_t st);
int wmf_launch_factorize(const double* G_sum, int f, int ld, double lambda, float* Wwhite, float* Wunwhite,
                         int32_t* info, double* gA, hipStream_t st, int perm = 0);   // perm: wmf_dense.hip, wmf_perm
int wmf_launch_transform(const float* in, int64_t m, int f, int ld, const float* W, int set_col0_one, float* out,
                         float* col0_out, hipStream_t st);
// the chained whitening of a solved side (wmf_dense.hip, "chained")
int wmf_launch_gram_aug(const float* g, int64_t m, int f, int ld, int bias, double* G_aug, float* partial, double* slices,
                        hipStream_t st);
int wmf_launch_compose(const double* G_aug, const float* U, int f, int ld, int bias, int flags, double lambda, float* Wwhite,
                       float* Wunwhite, float* N_ext, int32_t* info, double* scratch, double* gA, hipStream_t st);
int wmf_launch_transform_chained(const float* g, int64_t m, int f, int ld, int bias, const float* N_ext, int rolled, float* out,
                                 float* col0_out, hipStream_t st);

// ---- how a launch is routed ("How a launch is routed") --------------------------------------------------------------
// What a launcher answers; wmf_api.hip (launch_error) turns it into WMF_E* and the message.
enum WmfLaunchRc { WMF_L_OK = 0, WMF_L_NO_KERNEL = -1, WMF_L_HIP = -2, WMF_L_LAYOUT = -3, WMF_L_TOO_MANY_KEYS = -4 };

// What is the same for every launch of one wmf_solve_rows call.  Host only: a launch site unpacks it into the kernel's positional
// arguments.  side: NULL, or the {last feature, bias} pairs of the split layout (V is then the packed body); biasv / bstride: what
// the low-row and pivoted kernels read the biases from (the pairs again, or NULL once the biases are folded into vals);
// fb_rows / fb_count: the list of rows bounced to the pivoted kernel; dbg: wmf_debug_flags, read once per call;
// rolled: V / the pairs are in the rolled coordinates with the bias bits (wmf_solve_rows_ex(WMF_SOLVE_ROLLED))
struct RowArgs {
    const float* V; const float* side; const float* biasv; int bstride;
    const int64_t* indptr; const int32_t* indices; const float* vals;
    int f, ld; float* g; int32_t* fb_rows; int32_t* fb_count; int32_t* fail_count;
    int dbg; bool rolled; hipStream_t st;
};
// rows[0 .. count); count_dev: NULL, or the device-side number of rows -- count is then the capacity of the list and sizes the grid
// (the bounce list of wmf_iter.hip)
struct RowList { const int32_t* rows; int64_t count; const int32_t* count_dev; };

// A run-time block count as a template argument: fn(wmf_int<N>{}) for the N of the list that equals n (fn answers a WmfLaunchRc),
// WMF_L_NO_KERNEL when none does.  Exactly the listed N are instantiated.
template <int N>
using wmf_int = std::integral_constant<int, N>;
template <int... NS, class Fn>
static inline int wmf_dispatch_list(int n, Fn&& fn) {
    int rc = WMF_L_NO_KERNEL;
    (void)(... || (n == NS ? ((rc = fn(wmf_int<NS>{})), true) : false));   // (a left fold: the kernels are instantiated, and so emitted, in the order of the list)
    return rc;
}
template <int LO, class Fn, int... IS>
static inline int wmf_dispatch_seq(int n, Fn&& fn, std::integer_sequence<int, IS...>) { return wmf_dispatch_list<(LO + IS)...>(n, fn); }
template <int LO, int HI, class Fn>                              // LO <= n <= HI
static inline int wmf_dispatch_nfb(int n, Fn&& fn) { return wmf_dispatch_seq<LO>(n, fn, std::make_integer_sequence<int, HI - LO + 1>{}); }
// ... and the one-wave-per-row kernels' pair (wmf_directw.hip): m blocks and a border column where wmf_dw_border(f), m = 1, 2, 4, 5,
// 6, 8 -- the row stream delivers the border feature as its own dword block unless m + 1 is a multiple of 4 --, plain blocks elsewhere;
// fn(N, std::bool_constant<BORDER>{})
template <class Fn>
static inline int wmf_dispatch_dw(int f, bool border, Fn&& fn) {
    if (border) return wmf_dispatch_list<1, 2, 4, 5, 6, 8>(f / 16, [&](auto n) { return fn(n, std::true_type{}); });
    return wmf_dispatch_nfb<1, 9>((f + 15) / 16, [&](auto n) { return fn(n, std::false_type{}); });
}

int wmf_launch_solve(const wmf_plan* plan, const RowArgs& a);
static inline int wmf_direct_supported(int f) { return f >= 1 && f <= 144; }   // one wave per row holds the f x f system
// Widths whose last feature is a border column of an m-block system (f = 16 m + 1 <= 144, m + 1 not a multiple of 4;
// WMF_DBG_NO_BORDER, 256, switches the border off): k = 16 m with biases.
static inline bool wmf_dw_border(int f) { return f > 16 && f <= 144 && f % 16 == 1 && (f / 16) % 4 != 3 && !(wmf_debug_flags & WMF_DBG_NO_BORDER); }
// SPLIT LAYOUT of the whitened fixed side of a bias model at those widths (ld = f + 3): the first f - 1 = 16 m features of
// row i are a packed body row V[i * (f - 1) ..] -- 64 m bytes, whole 128-byte lines when m is even, where an (f + 3)-float
// row at a 528-byte stride (f = 129) touched five lines for 4.03 lines of data -- and the last feature and the side's bias are
// the pair side[2 i], side[2 i + 1] of a small second array (8 bytes per row: 8 MB for a million items, resident in L2 /
// Infinity Cache).  The row kernels subtract the bias from the entry weights as it arrives (RecModel/wmf_model.py:343): no
// separate pass over all entries.  Written by wmf_row_transform(set_col0_one = 1), read by every row kernel of
// wmf_solve_rows / wmf_accumulate_rows when a bias array is given.
static inline bool wmf_split_layout(int f, int ld) { return wmf_dw_border(f) && ld == f + 3; }
// wmf_directl.hip: normal heavy rows at f = 128 / 129 through an LDS-DMA row ring
int wmf_directl_supported(int f, int ld);
int wmf_launch_directl(const RowArgs& a, RowList l);
// (the segments of the plan's split rows, partial systems into pl->partial)
int wmf_launch_directl_segments(const wmf_plan* pl, const RowArgs& a);
int wmf_launch_directw(const wmf_plan* pl, const RowArgs& a);
int64_t wmf_directw_partial_floats(int f);
// reduce mode: partial systems of the n rows of a CSR (degrees[r] entries from indptr[r]) into slot r * slot_stride + slot_offset;
// elimination of n summed systems of slots_per_row slots each.  Of `a` they read what their kernels take.
int wmf_launch_accumulate(const RowArgs& a, const int32_t* degrees, int64_t n, float* partial, int slot_stride, int slot_offset);
int wmf_launch_eliminate(const RowArgs& a, float* partial, int64_t n, int slots_per_row);
void wmf_launch_bias_adjust(const float* vals, const int32_t* indices, const float* biasv, int64_t nnz, float* w_eff,
                            hipStream_t st);
// wmf_csr.hip: COO -> CSR, stable in (row, column)
int64_t wmf_csr_ws_bytes(int64_t nnz, int64_t n_rows, int64_t n_cols);
int wmf_launch_coo_to_csr(const int64_t* rows, const int64_t* cols, const float* vals, int64_t nnz, int64_t n_rows, int64_t n_cols,
                          int64_t* indptr, int32_t* indices, float* values, int32_t* bad_flag, void* ws, hipStream_t st);
int wmf_wide_supported(int f);
int wmf_launch_wide(const RowArgs& a, RowList l);
// wmf_iter.hip: rows with 33 .. wmf_iter_dmax entries whose whitened system is close to the identity, by a matrix-free
// Neumann / Chebyshev iteration; the rows it does not solve are appended to bounce_rows (count on the device)
int wmf_iter_dmax(int f, int ld, int split);
// (l: candidates, the first rows of the plan's bin; the plan holds the bounce list, its counters and the candidates' records)
int wmf_launch_iter(const wmf_plan* pl, const RowArgs& a, RowList l);
static inline bool wmf_iter_enabled() { return !(wmf_debug_flags & WMF_DBG_NO_ITER); }
// The rolled whitened coordinates with the bias in the body's last mantissa bits (include/wmf_hip.h, wmf_row_transform modes 3 / 4,
// wmf_solve_rows_ex): bias models whose packed body is 128 floats (k = 128), transform6_kernel and the iteration kernels only
// (a lab build's f32 transform_kernel, WMF_DBG_F32_TRANSFORM, cannot write it)
static inline bool wmf_rolled_layout(int f, int ld) {
    return f == 129 && wmf_split_layout(f, ld) && !(wmf_debug_flags & (WMF_DBG_F32_TRANSFORM | WMF_DBG_NO_ROLLED_LAYOUT));
}
// candidates of this call: none when the iteration is switched off, or when the call's layout (ld, split) is not the one the
// plan sorted its rows for (a caller with its own leading dimension: the kernel's register slots would not hold the rows)
static inline int64_t wmf_iter_rows(const wmf_plan* pl, int f, int ld, bool split) {
    return (wmf_iter_enabled() && pl->iter_count > 0 && wmf_iter_dmax(f, ld, split ? 1 : 0) >= pl->iter_dmax) ? pl->iter_count : 0;
}
int wmf_rowsplit_supported(int f);
int wmf_launch_rowsplit(const wmf_plan* pl, const RowArgs& a);
int64_t wmf_rowsplit_partial_floats(int f);      // floats of one segment's partial system
// partial systems of the segments of every split row summed, in segment order, into the row's first slot (wmf_solve.hip)
void wmf_launch_combine_segments(const wmf_plan* pl, int64_t partial_floats, hipStream_t st);
// The schedule of the plan's bin of rows with more than 32 entries, once for every kernel family that solves it (directw with
// its directl choice, rowsplit, wide): the iteration's candidates; the rows that were never candidates (count on the host); the
// rows it bounced (count on the device: the grid is sized for the list's capacity and exits at once when the list is empty);
// then the `heavy` last rows of the bin as segments -> combine -> eliminate.  launch(mode, list) runs the family's kernel:
// mode 0 solves the rows of the list, 1 writes the partial systems of the plan's segments (the list counts them), 2 eliminates
// the heavy rows; partial_floats is the size of one segment's partial system.
template <class Launch>
static inline int wmf_schedule_bin(const wmf_plan* pl, int bin, const RowArgs& a, int64_t heavy, int64_t partial_floats, Launch&& launch) {
    const int32_t* rows = pl->rows[bin];
    const int64_t normal = pl->count[bin] - heavy;
    // ROUND 4: the first iter_count of the normal rows (at most wmf_iter_dmax entries each, wmf_plan_create) go to the
    // matrix-free iteration kernel (wmf_iter.hip); what it cannot solve to float32 accuracy in a few applications of the
    // row's operator comes back as a device-side list and is eliminated like every other row.  WMF_DBG_NO_ITER (268435456)
    // switches the iteration off (everything eliminated, as in round 3).
    // (f > 144: the kernels of that bin know no split layout, and biasv is always folded into vals by wmf_launch_solve)
    const int64_t n_iter = bin == WMF_BIN_GENERAL ? (a.biasv ? 0 : wmf_iter_rows(pl, a.f, a.ld, false)) : wmf_iter_rows(pl, a.f, a.ld, a.side != nullptr);
    int rc = WMF_L_OK;
    if (n_iter > 0 && (rc = wmf_launch_iter(pl, a, RowList{rows, n_iter, nullptr}))) return rc;
    if (normal > n_iter && (rc = launch(0, RowList{rows + n_iter, normal - n_iter, nullptr}))) return rc;
    if (n_iter > 0 && (rc = launch(0, RowList{pl->iter_bounce_rows, n_iter, pl->fallback_count + 1}))) return rc;
    if (heavy > 0) {
        if ((rc = launch(1, RowList{rows, pl->seg_total, nullptr}))) return rc;
        wmf_launch_combine_segments(pl, partial_floats, a.st);
        rc = launch(2, RowList{rows + normal, heavy, nullptr});
    }
    return rc;
}
size_t wmf_wide_lu_workspace_bytes(int f);
// (the rows of the bounce list a.fb_rows / a.fb_count)
int wmf_launch_wide_lu(const RowArgs& a, float* work);
int wmf_launch_spmm(const float* V, const int64_t* indptr, const int32_t* indices, const float* values, int64_t n,
                    int ld, float* g, hipStream_t st);
int wmf_launch_eval(const float* users, const float* items, int f, int ld, int bias, const int64_t* indptr,
                    const int32_t* indices, const float* values, int64_t n, double* out3, double* partial,
                    hipStream_t st);
// wmf_audit.hip: objective sums and per-row backward-error terms of a half step, float32 and float64 factors
int64_t wmf_audit_ws_bytes(int64_t n);
int wmf_launch_audit(const float* X, const float* Y, int f, int ld, int bias, const int64_t* indptr, const int32_t* indices,
                     const float* values, int64_t n, const double* dense, double* out_sums, double* out_rows, void* ws, hipStream_t st);
int wmf_launch_audit_f64(const double* X, const double* Y, int f, int bias, const int64_t* indptr, const int32_t* indices,
                         const double* values, int64_t n, const double* dense, double* out_sums, double* out_rows, void* ws, hipStream_t st);
// wmf_explain.hip: per-entry contributions of a row's history to the scores of target items
int wmf_launch_explain(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                       const float* values, int64_t n, const int32_t* targets, int n_targets, float* out_contrib, float* out_total,
                       int32_t* fail_count, hipStream_t st);
// wmf_foldin.hip: the folded-in factors of a row's history (the x_u whose scores wmf_explain.hip splits up)
int wmf_launch_foldin(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                      const float* values, int64_t n, float* X_out, int32_t* fail_count, hipStream_t st);
// wmf_posterior.hip: draws from the posterior of a folded-in row, mean and variance of its scores, and the noise of arbitrary
// (stream, draw, component) triples
int wmf_launch_posterior_draw(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                              const float* values, int64_t n, int n_draws, float sigma, uint64_t seed, const uint64_t* row_stream,
                              float* X_out, int32_t* fail_count, hipStream_t st);
int wmf_launch_posterior_score(const float* Y, int f, int ld, int bias, const float* W, const int64_t* indptr, const int32_t* indices,
                               const float* values, int64_t n, const int32_t* targets, int n_targets, float* out_mean, float* out_var,
                               int32_t* fail_count, hipStream_t st);
void wmf_launch_posterior_noise(uint64_t seed, const uint64_t* row_stream, const int32_t* draws, const int32_t* components, int64_t n,
                                float* out_xi, uint32_t* out_k1k2, hipStream_t st);
int wmf_launch_predict(const float* users, const float* items, int f, int ld, int bias, const int32_t* ui, int64_t n_u,
                       const int32_t* ii, int64_t n_i, float* out, hipStream_t st);
int wmf_launch_hits(const float* users, const float* items, int ld, int bias, const int32_t* pair_user,
                    const int32_t* pair_item, const int32_t* pair_row, int64_t n_pairs, const int32_t* cand, int n_cand,
                    const int32_t* slot, const int32_t* topn, int n_topn, int64_t* hits, hipStream_t st);
int64_t wmf_rank_ws_bytes(int64_t n);
int wmf_launch_rank(const float* users, const float* items, int f, int ld, int bias, const int32_t* user_idx,
                    const int32_t* cand, int64_t n, int64_t topn, int32_t* out_pos, float* out_scores, void* ws, hipStream_t st);
int64_t wmf_rank_batch_ws_bytes(int64_t nu, int64_t nc);
int wmf_launch_rank_batch(const float* users, const float* items, int f, int ld, int bias, const int32_t* user_idx, int64_t nu,
                          const int32_t* cand, int64_t nc, int64_t topn, int32_t* out_pos, float* out_scores, void* ws, hipStream_t st);
// wmf_recommend.hip: full-catalogue top-n with per-user exclusions (workspace: n_slices = 0 is sized for the automatic cap)
int64_t wmf_recommend_ws_bytes(int64_t n_users, int64_t topn, int32_t n_slices);
// (flt, here and below: what restricts a row's list -- seen lists, allow masks or a list of n_cand candidate rows, the row itself;
// the empty filter is the unfiltered call)
int wmf_launch_recommend(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users,
                         int64_t n_items, const WmfRowFilter& flt, int64_t n_cand, int64_t topn, int32_t n_slices, int32_t* out_items,
                         float* out_scores, int32_t* out_count, void* ws, hipStream_t st);
// (the sorted partial lists of a scan with the top-n epilogue of wmf_topn.h, n_slices a row, merged into the outputs)
void wmf_launch_topn_merge(const unsigned long long* partial, int64_t n_rows, int n_slices, int topn, int32_t* out_rows, float* out_scores,
                           int32_t* out_count, hipStream_t st);
// (the slices of a scan over n_items for n_users rows: n_slices itself, or the automatic choice for 0; wmf_rankpos.hip cuts alike)
int wmf_recommend_slices(int64_t n_users, int64_t n_items, int64_t topn, int32_t n_slices);
// (... for 1 <= topn <= WMF_RECOMMEND_WIDE_MAX_TOPN: the keys of a row and slice in the workspace; any of the three forms)
int64_t wmf_recommend_wide_ws_bytes(int64_t n_users, int64_t topn, int32_t n_slices);
int wmf_recommend_wide_slices(int64_t n_users, int64_t n_scan, int64_t topn, int32_t n_slices);
int64_t wmf_recommend_wide_lists(int64_t n_users, int32_t n_slices);     // L of the workspace formula (n_slices = 0: the automatic L0)
int wmf_launch_recommend_wide(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users,
                              int64_t n_items, const WmfRowFilter& flt, int64_t n_cand, int64_t topn, int32_t n_slices, int32_t* out_items,
                              float* out_scores, int32_t* out_count, void* ws, hipStream_t st);
// (... one list per (row, group) from one scan: group_of[j] = the group of item j, the mask form or no filter)
int64_t wmf_recommend_grouped_ws_bytes(int64_t n_users, int32_t n_groups, int64_t topn, int32_t n_slices);
int wmf_recommend_grouped_slices(int64_t n_users, int64_t n_items, int32_t n_groups, int64_t topn, int32_t n_slices);
int wmf_launch_recommend_grouped(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users,
                                 int64_t n_items, const WmfRowFilter& flt, const int32_t* group_of, int32_t n_groups, int64_t topn,
                                 int32_t n_slices, int32_t* out_items, float* out_scores, int32_t* out_count, void* ws, hipStream_t st);
// wmf_sample.hip: the sampled top-n (the wide scan with Gumbel-perturbed keys; workspace and slices: wmf_recommend_topn_wide's), the
// log-partition of a row's eligible catalogue, and the noise of arbitrary (stream, item) pairs
int wmf_launch_sample(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_users, int64_t n_items,
                      const WmfRowFilter& flt, int64_t n_cand, int64_t topn, int32_t n_slices, float temperature, uint64_t seed,
                      const uint64_t* row_stream, int32_t* out_items, float* out_scores, float* out_keys, int32_t* out_count, void* ws,
                      hipStream_t st);
int64_t wmf_log_partition_ws_bytes(int64_t n_rows, int32_t n_slices);
int wmf_launch_log_partition(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_rows, int64_t n_items,
                             const WmfRowFilter& flt, int64_t n_cand, float temperature, int32_t n_slices, float* out_logz,
                             int32_t* out_eligible, void* ws, hipStream_t st);
void wmf_launch_sample_noise(uint64_t seed, const uint64_t* row_stream, const int32_t* items, int64_t n_pairs, float* out_g, uint32_t* out_k,
                             hipStream_t st);
// wmf_similar.hip: inverse row norms, and the neighbours of rows of one factor matrix among the rows of another (dot or cosine)
void wmf_launch_row_inv_norms(const float* M, int64_t n, int f, int ld, int bias, float* out, hipStream_t st);
int wmf_launch_similar(const float* queries, const float* catalogue, int ld, int bias, const float* q_inv_norm, const float* c_inv_norm,
                       const int32_t* query_idx, int64_t n_queries, int64_t n_rows, const WmfRowFilter& flt, int64_t topn, int32_t n_slices,
                       int32_t* out_rows, float* out_scores, int32_t* out_count, void* ws, hipStream_t st);
// wmf_mmr.hip: greedy MMR re-ranking of a row's candidate pool (the resident kernel for pool <= wmf_mmr_resident_pool, the
// streaming one beyond), and the intra-list similarity of finished lists
int64_t wmf_mmr_resident_pool(int f, int ld);
int wmf_launch_mmr(const float* items, int64_t n_items, int f, int ld, int bias, const float* inv_norm, const int32_t* pool_items,
                   const float* pool_scores, const int32_t* pool_count, int64_t n_rows, int64_t pool, float lambda, int64_t topn,
                   int32_t* out_items, float* out_scores, float* out_marginal, int32_t* out_count, hipStream_t st);
int wmf_launch_ils(const float* items, int64_t n_items, int f, int ld, int bias, const float* inv_norm, const int32_t* lists,
                   const int32_t* list_count, int64_t n_rows, int64_t width, float* out_mean, float* out_max, hipStream_t st);
// wmf_rankpos.hip: exact full-catalogue ranks of target items, seen items left out
int64_t wmf_rank_positions_ws_bytes(int64_t n_rows);
int wmf_launch_rank_positions(const float* users, const float* items, int ld, int bias, const int32_t* user_idx, int64_t n_rows,
                              int64_t n_items, const int64_t* seen_indptr, const int32_t* seen_indices, const int64_t* target_indptr,
                              const int32_t* target_indices, int32_t n_slices, int32_t* out_rank, float* out_score, void* ws, hipStream_t st);
int wmf_launch_gather_rows(const float* in, int ld, const int64_t* rows, int64_t n, float* out, hipStream_t st);
int wmf_launch_confidence(float* values, int64_t nnz, double alpha, double beta, int mode, hipStream_t st);
// float64 half step of the cores > 1 variants (wmf_f64.hip)
int64_t wmf_f64_ws_bytes(int f, int64_t m, int64_t n);
int wmf_launch_half_step_f64(const double* Y, int64_t m, int f, int bias, const int64_t* indptr, const int32_t* indices,
                             const double* values, int64_t n, double lambda, double* X, void* ws, int32_t* fail, hipStream_t st);
int wmf_launch_confidence_f64(double* values, int64_t nnz, double alpha, double beta, int mode, hipStream_t st);
// wmf_iter64.hip: the matrix-free iteration in float64 (rows of 1 .. 32 entries: low = 1; 33 .. wmf_iter64_dmax: low = 0)
int wmf_iter64_dmax(int f);
int wmf_launch_iter64(const double* V, const double* Y, int f, int bias, const int64_t* indptr, const int32_t* indices,
                      const double* vals, int64_t n, int low, double* gout, int32_t* state, const int32_t* ctrl, hipStream_t st);

void wmf_set_error(const char* fmt, ...);
int wmf_cu_count();                              // compute units of the current device (wmf_api.hip)
// Ablation switches whose results are WRONG (WMF_DBG_NO_ELIMINATION, _NO_ACCUMULATION, _NO_TILE_INVERSE) are compiled
// into a -DWMF_LAB build only; the shipped library has no such code path.
#ifdef WMF_LAB
#define WMF_ABL(dbg, bits) ((dbg) & (bits))
#else
#define WMF_ABL(dbg, bits) 0
#endif

// per-kernel event timing (wmf_api.hip).  A launch site names its kernel the way rocprofv3 prints the symbol, up to and
// including the template arguments ("solve_low_kernel<9, 1, false, false>"), so that bench.py's table and a
// rocprofv3 --kernel-trace --stats summary of the same run can be matched line by line.
const char* wmf_kname(const char* fmt, ...);     // interned: the pointer stays valid for the life of the library
// a kernel's name and the name of its launch over a device-counted list of bounced rows (a separate line of the timing table)
struct WmfKName {
    const char* plain; const char* bounced;
    const char* of(const RowList& l) const { return l.count_dev ? bounced : plain; }
};
WmfKName wmf_kname_pair(const char* fmt, ...);   // {name, name + " [bounced]"}, interned
static inline const char* wmf_tf(bool b) { return b ? "true" : "false"; }   // a bool template argument as rocprofv3 prints it
void wmf_prof_begin(const char* name, hipStream_t st);
void wmf_prof_end(hipStream_t st);
struct WmfProfScope {
    hipStream_t st;
    WmfProfScope(const char* name, hipStream_t s) : st(s) { wmf_prof_begin(name, s); }
    ~WmfProfScope() { wmf_prof_end(st); }
};
#define WMF_LAUNCH(NAME, KERNEL, GRID, BLOCK, LDS, ST, ...)                          \
    do {                                                                             \
        WmfProfScope wmf_ps_(NAME, ST);                                              \
        hipLaunchKernelGGL(KERNEL, GRID, BLOCK, LDS, ST, __VA_ARGS__);               \
    } while (0)
// The ceiling of a kernel's dynamic LDS, raised once per kernel, at the first pass over the statement (a function-local static's
// initialiser: thread-safe), and WMF_LAUNCH behind it.
static inline bool wmf_lds_ceiling(const void* kernel, size_t bytes) {
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return true;
}
#define WMF_LDS_CEILING(KERNEL, BYTES)                                                        \
    do {                                                                                      \
        static const bool wmf_lc_ = wmf_lds_ceiling((const void*)KERNEL, BYTES);              \
        (void)wmf_lc_;                                                                        \
    } while (0)
#define WMF_LAUNCH_LDS(NAME, KERNEL, CEILING, GRID, BLOCK, LDS, ST, ...)                      \
    do {                                                                                      \
        WMF_LDS_CEILING(KERNEL, CEILING);                                                     \
        WMF_LAUNCH(NAME, KERNEL, GRID, BLOCK, LDS, ST, __VA_ARGS__);                          \
    } while (0)
