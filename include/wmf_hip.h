/* wmf_hip.h -- C ABI of libwmf_hip.so: MI355X (gfx950) kernels for the WMF/ALS hot path.
 *
 * The reference (titoeb/RecModel) has no FFI or operator interface for this path: the seam is
 * the pair of pure functions
 *
 *     WMF.recompute_factors(Y, C, lambda_reg)            RecModel/wmf_model.py:213-240
 *     WMF.recompute_factors_bias(Y, C, lambda_reg, ...)  RecModel/wmf_model.py:311-351
 *
 * plus WMF.predict (wmf_model.py:191-211) as used by RecModel.eval_prec (base_model.py:150-179).
 * This header declares what a ctypes / cffi binding for those functions binds.  INTEGRATION.md
 * shows the reference-side stub.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative WMF_E* code, and
 *     wmf_last_error() returns a message for the calling thread's last failure.
 *   - "host" entry points take host pointers and are self-contained (own hipMalloc/copies).
 *   - "device" entry points take device pointers and a hipStream_t passed as void*; they only
 *     enqueue work (no allocation, no synchronisation) so a caller can keep factors resident in
 *     HBM across half steps and put collectives between them.  Whatever device memory a solve needs
 *     beyond the caller's buffers is allocated by wmf_plan_create and freed by wmf_plan_destroy.
 *   - factor matrices are row-major fp32 with a leading dimension `ld` (floats), ld % 4 == 0,
 *     ld >= f; the padding columns [f, ld) must be zero on input and are written as zero.
 *     f = k (no bias) or k+1 (bias: column 0 is the bias, wmf_model.py:328-331).
 *   - CSR is consumed "as stored": stored zeros contribute, duplicates are not merged
 *     (wmf_model.py:231-239).  indptr is int64, indices int32, values fp32.
 */
#ifndef WMF_HIP_H
#define WMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WMF_OK            0
#define WMF_EINVAL       -1   /* bad argument (shape, alignment, unsupported f)           */
#define WMF_EHIP         -2   /* a HIP runtime call failed                                */
#define WMF_ENOMEM       -3   /* allocation failed                                        */
#define WMF_ENUMERIC     -4   /* Gramian not positive definite / singular row system      */

#define WMF_MAX_F        260  /* largest supported factor width (k = 256 + bias, padded)  */

typedef struct wmf_plan wmf_plan;   /* opaque: degree-binned row schedule of one CSR matrix */

/* ---- library ---------------------------------------------------------------------------- */
const char* wmf_last_error(void);
int  wmf_version(void);
/* Smallest legal leading dimension for factor width f (round up to a multiple of 4). */
int  wmf_ld_for(int f);

/* ---- host-level drop-in for the operator seam -------------------------------------------- */
/* X_new = recompute_factors[_bias](Y, C, lambda)          wmf_model.py:213-240 / 311-351
 *   Y_host   [m, f]  row-major contiguous fp32 (bias != 0: column 0 is the fixed side's bias)
 *   C        CSR [n, m]: indptr int64[n+1], indices int32[nnz], values fp32[nnz]
 *   X_host   [n, f]  output, row-major contiguous fp32
 * Runs on the current HIP device; synchronous. */
int wmf_recompute_factors_host(const float* Y_host, int64_t m, int f, int bias,
                               const int64_t* indptr, const int32_t* indices, const float* values,
                               int64_t n, double lambda, float* X_host);

/* ---- device-level building blocks (resident training loop) ------------------------------- */
/* Workspace (device, caller-allocated) needed by the Gramian + factorisation step. */
int64_t wmf_gram_workspace_bytes(int f);

/* Partial Gramian of a (shard of a) factor matrix:  G_sum[f*f] (fp64, row-major) =
 * sum_r y~_r y~_r^T over the m rows given, where y~ = y with column 0 replaced by 1 when
 * bias != 0 (wmf_model.py:331-332).  No lambda yet: multi-GPU callers all-reduce G_sum first.
 * wmf_model.py:215 (np.dot(Y.T, Y)). */
int wmf_gram(const float* Y, int64_t m, int f, int ld, int bias,
             double* G_sum, void* workspace, void* stream);

/* From the (all-reduced) Gramian: A = G_sum + lambda*I = L L^T (fp64, on device) and the two
 * fp32 transforms used by the row solve, both [f, ld] row-major, zero padded:
 *   W_white[a][b]   = (L^-T)[a][b]     V = Y~ . W_white      (whitened fixed factors)
 *   W_unwhite[a][b] = (L^-1)[a][b]     X = g  . W_unwhite    (back to factor space)
 * info (device int32, caller zeroes): left alone on success, set to j > 0 when leading minor j is not positive
 * definite -- sticky, so one check after several half steps still sees a failure of the first (the outputs of a
 * failed factorisation are zero matrices).
 * Replaces the `+ lambda_reg * np.eye(...)` of wmf_model.py:215/332 and the shared part of the
 * per-row np.linalg.solve of :239/:350. */
int wmf_factorize(const double* G_sum, int f, int ld, double lambda,
                  float* W_white, float* W_unwhite, int32_t* info,
                  void* workspace, void* stream);

/* out[r, :] = in~[r, :] . W  for rows [0, m), in/out [m, ld], W [f, ld]; padding columns are written as zero.
 * set_col0_one != 0 (whitening of the fixed side of a bias model): in~ is `in` with column 0 read as 1, and the bias
 * in[r,0] (wmf_model.py:328-331) is copied to col0_out[r] (may be NULL).
 * out == in (in place) is allowed wherever out has the layout of in -- every call but the split-layout and rolled whitening
 * below: a wave reads its 16 rows whole before it writes them (for f > 176 W is then read from global memory, one launch
 * instead of the column slices: slower, same arithmetic; tests/test_gpu_dense.py runs it at every block count).
 * SPLIT LAYOUT.  For the widths with wmf_whitened_row_floats(f, ld, 1) == f - 1 -- f = 16 m + 1 <= 144 with ld = f + 3:
 * k = 16, 32, 64, 80, 96, 128 with biases -- set_col0_one != 0 writes the whitened side in the form the row kernels gather
 * cheapest: out is a PACKED body, out[r * (f - 1) + c] = feature c < f - 1 of row r (64 m bytes a row, whole 128-byte lines,
 * where the (f + 3)-float row at its 528-byte stride touched five lines for 4.03 lines of data), and col0_out, then
 * REQUIRED, is float[2 m]: col0_out[2 r] = feature f - 1, col0_out[2 r + 1] = the bias.  out may not alias in there.
 * wmf_solve_rows / wmf_accumulate_rows take the two arrays as their V and bias_fixed. */
/* ROLLED COORDINATES (round 4; wmf_rolled_layout_supported(f, ld) != 0: bias models with a 128-float body, k = 128).  With a
 * bias model whitened feature 0 is the same number for every row -- in~'s column of ones times an upper-triangular W_white -- so
 * a caller may keep the whitened side in coordinates rolled by one: feature c at position c - 1, feature 0 last.
 *   set_col0_one = 3  whitening as above (split layout), written in rolled coordinates: the border feature of the pairs is
 *                     then that constant, and the 32 bits of the row's bias replace the last mantissa bit of body positions
 *                     8 j, 8 j + 1 (j < 16; each value moves by at most one ulp).  The row kernels that hold eight consecutive
 *                     features per lane rebuild the bias from the row they gathered: the pairs -- 8 bytes that cost a whole
 *                     128-byte line per stored entry, 1.0 - 1.9 ms of configs[2]'s item half step -- are not fetched at all.
 *   set_col0_one = 4  the input is in rolled coordinates (the g of wmf_solve_rows_ex(WMF_SOLVE_ROLLED)): out = in . W as for 0.
 * Every kernel accepts such a V / pairs (it is a permutation of the features); wmf_solve_rows_ex must be told, because the
 * kernels that skip the pairs rely on both properties. */
int wmf_rolled_layout_supported(int f, int ld);

int wmf_row_transform(const float* in, int64_t m, int f, int ld, const float* W,
                      int set_col0_one, float* out, float* col0_out, void* stream);
/* Floats per row of the whitened fixed side that wmf_row_transform(set_col0_one = bias) writes and the row kernels read:
 * ld, or f - 1 for the split layout above (0: f, ld not supported). */
int wmf_whitened_row_floats(int f, int ld, int bias);

/* ---- CHAINED WHITENING of a side that was just solved (f = 97 .. 144) ----
 * The factors X = g . U (U = the W_unwhite that un-whitens g) are an exact linear image of g, so the Gramian and the whitened
 * rows the NEXT half step needs of this side follow from g and two small matrices, without X being written or read.  With
 * a = [g, 1] (bias != 0; the one at position f of a row, which ld >= f + 1 has room for) or a = g, and T the (f + bias) x f
 * matrix with rows 0 .. f - 1 = U, column 0 zeroed, and row f = e0^T (T = U without biases):
 *     in~ = a . T,   G~ = T^T (a^T a) T = wmf_gram(X, bias),   V = a . (T . W_white),   bias = g . U[:, 0].
 * All three calls take a workspace of wmf_gram_workspace_bytes(f + 1).  g's padding columns are not read as data.
 * wmf_chained_supported: non-zero where the three are implemented -- f = 97 .. 144 with f + bias <= 144 and ld >= f + bias. */
int wmf_chained_supported(int f, int ld, int bias);
/* G_aug[(f + bias)^2] (fp64, row-major) = a^T a over the m rows of g (g in rolled coordinates or not: positions). */
int wmf_gram_whitened(const float* g, int64_t m, int f, int ld, int bias,
                      double* G_aug, void* workspace, void* stream);
/* On the device, fp64, no host synchronisation: G~ = T^T G_aug T, then wmf_factorize(G~, lambda) -> W_white, W_unwhite, info
 * (its semantics and rounding), then N_ext [(f + bias), ld] fp32 = [T . W_white | U[:, 0]] (column f: the bias; padding zero).
 * rolled != 0 (wmf_rolled_layout_supported): g came from wmf_solve_rows_ex(WMF_SOLVE_ROLLED) and the whitened side is wanted
 * in rolled coordinates -- row p of N_ext belongs to position p of g, column n to position n of the whitened row.
 * `rolled` is a set of flags: 0 and 1 (WMF_COMPOSE_ROLLED) are the two values above.  WMF_COMPOSE_REVERSED (2) factorises
 * P^T (G~ + lambda I) P = L L^T with P = diag(1, J) (bias; J reverses features 1 .. f - 1) or P = J (no bias: all f features)
 * and returns W_white = P L^-T, W_unwhite = L^-1 P^T = W_white^T: a whitening as valid as L^-T (W_white^T (G~ + lambda I)
 * W_white = I, whitened feature 0 of a bias model still the constant 1 / L[0][0]), whose matrices are anti-triangular in
 * feature order.  Where exactly one of two consecutive half steps sets the flag, N_ext[i][j] = 0 for i + j < f (bias: i the
 * feature at a position of g, j the whitened feature; the row of the one and the bias column are dense; i + j < f - 1 without
 * biases), so wmf_row_transform_chained skips those tiles.  The solved factors do not depend on the choice but for rounding.
 * U [f, ld] may not alias W_white / W_unwhite. */
#define WMF_COMPOSE_ROLLED 1
#define WMF_COMPOSE_REVERSED 2
int wmf_compose_whitening(const double* G_aug, const float* U, int f, int ld, int bias, int rolled, double lambda,
                          float* W_white, float* W_unwhite, float* N_ext, int32_t* info,
                          void* workspace, void* stream);
/* out / col0_out = a . N_ext in exactly the layout wmf_row_transform(X, W_white, set_col0_one = bias, or 3 when rolled)
 * writes: plain rows and the bias vector, the split layout, or the rolled split layout with the bias bits in the body. */
int wmf_row_transform_chained(const float* g, int64_t m, int f, int ld, int bias, const float* N_ext, int rolled,
                              float* out, float* col0_out, void* stream);

/* Degree-binned schedule for the rows of one CSR matrix (built once per matrix, host indptr).  Allocates (and
 * synchronously fills) the plan's device memory, including everything wmf_solve_rows will need: the row lists, the
 * segment table of rows with more than 4096 entries, with bias != 0 the bias-adjusted weights (one float per stored
 * entry, wmf_model.py:343), for f > 144 the workspace of the pivoted fallback.  A plan created with bias = 0 cannot
 * be solved with a bias vector. */
int  wmf_plan_create(const int64_t* indptr_host, int64_t n, int f, int bias, wmf_plan** out);
void wmf_plan_destroy(wmf_plan* p);
/* Rows and stored entries the plan routes to each kernel family: out12[b] = rows, out12[4+b] =
 * stored entries, for b = 0: <=16 entries, 1: 17..32, 2: one wave per row (f <= 144), 3: four waves per row (f > 144);
 * out12[8], out12[9] = rows and entries of bin 0 with at most 8 entries (two rows share a wave);
 * out[10], out[11] = rows and entries of bin 2 / 3 with more than 4096 entries (split over several waves);
 * out[12], out[13] = rows and entries of bin 2 / 3 that are candidates of the matrix-free iteration kernel (33 .. a
 * width-dependent number of entries; round 4).  The array has 14 elements. */
int  wmf_plan_stats(const wmf_plan* p, int64_t* out14);
/* What became of those candidates in the solves since the last call: out4 = { rows solved by the iteration, rows handed
 * back to the elimination kernels (bound on the row's operator too weak, or no convergence), applications of the row
 * operator in total, rows solved by the Chebyshev rather than the Neumann recurrence }.  Data dependent: a row is solved
 * by a truncated polynomial in E = V_u^T D V_u only when tr E bounds it away from the direct method's cost
 * (csrc/wmf_iter.hip).  Synchronises the device and clears the counters. */
int  wmf_plan_iter_stats(wmf_plan* p, int64_t* out4);

/* The per-row normal-equation solve in whitened coordinates, for every row of the CSR:
 *   g_u = (I + V_u^T D_u V_u)^-1 V_u^T (w_u + 1),   V_u = V[idx_u], D_u = diag(w_u)
 * with w_u = values - bias_fixed[idx_u] when bias_fixed != NULL (wmf_model.py:343).  V and bias_fixed must both come
 * from wmf_row_transform(set_col0_one = 1) on the same matrix (for the widths named there: packed body and pairs; the
 * kernels then take the bias with the gathered row, elsewhere one pass over the entries folds it into the weights).
 * g [n, ld]; follow with wmf_row_transform(g, W_unwhite) to obtain X_new.
 * Restates the loop body wmf_model.py:220-239 / 337-350.  Rows without stored entries give 0.
 * fail_count (device int32, caller zeroes): number of rows whose system was numerically singular. */
int wmf_solve_rows(const wmf_plan* plan, const float* V, const float* bias_fixed,
                   const int64_t* indptr, const int32_t* indices, const float* values,
                   int64_t n, int f, int ld, float* g, int32_t* fail_count, void* stream);
/* The same, with flags: WMF_SOLVE_ROLLED = V and bias_fixed come from wmf_row_transform(set_col0_one = 3) (see there); g is
 * then in rolled coordinates: follow with wmf_row_transform(g, W_unwhite, set_col0_one = 4). */
#define WMF_SOLVE_ROLLED 1
int wmf_solve_rows_ex(const wmf_plan* plan, const float* V, const float* bias_fixed,
                   const int64_t* indptr, const int32_t* indices, const float* values,
                   int64_t n, int f, int ld, float* g, int32_t* fail_count, int flags, void* stream);

/* Sum over the stored, non-zero entries of a CSR "utility" matrix of (value - predict(u, i))^2
 * and |value - predict(u, i)| -- RecModel.eval_prec (base_model.py:163-176) with WMF.predict
 * (wmf_model.py:205-211).  The CSR has n user rows; `users` is the matching [n, ld] factor block
 * (a multi-GPU caller passes its own user shard and the shard's CSR), `items` the full item
 * matrix.  Stored zeros are skipped (utility_mat.nonzero(), base_model.py:163).
 * out3 (device fp64[3]) = { sum of squares, sum of abs, count }.
 * workspace: device, wmf_eval_workspace_bytes() bytes. */
int64_t wmf_eval_workspace_bytes(void);
int wmf_eval_sqerr(const float* users, const float* items, int f, int ld, int bias,
                   const int64_t* indptr, const int32_t* indices, const float* values,
                   int64_t n, double* out3, void* workspace, void* stream);

/* ---- audit of a half step: its objective and the backward error of every row ------------------------------------------
 * One pass over the CSR of the half step that updated side R (rows x_u, X [n, ld]) against the fixed side F (Y), in float64
 * on the factors as stored and independent of every solver path.  The CSR is read as stored (stored zeros count, duplicates
 * are separate entries).  With y~_i = row i of F with column 0 read as 1 when bias != 0 and beta_i = F[i, 0] when bias != 0,
 * else 0 (wmf_model.py:253-257, :279, :328-343), every stored entry e = (u, i, c) has
 *     w = c - beta_i,      s = x_u . y~_i over all f columns  (not predict: with biases x_u[0] multiplies the 1)
 * and the call returns
 *     out_sums = { S1 = sum_e (1 + w)(1 - s)^2,  S2 = sum_e s^2,  N = number of entries }
 *     out_rows[u] = { |r_u|^2, |b_u|^2, a_u }   (squared 2-norms: integer inputs stay exact)
 *         r_u = dense_u + sum_e [w s - (w + 1)] y~_i,   dense_u = (G~ + lambda I) x_u supplied by the caller,
 *                                                       G~ = sum_i y~_i y~_i^T = what wmf_gram(bias) returns
 *         b_u = sum_e (w + 1) y~_i,      a_u = sum_e |w| |y~_i|^2
 * r_u = A_u x_u - b_u for the A_u, b_u of wmf_model.py:237-239 and :343-350, so
 *     objective of the half step   L     = <X^T X, G~>_F + S1 - S2 + lambda |X|_F^2   (the first term: s^2 over ALL pairs; every
 *                                          row of the reference's half step minimises its share of L)
 *     normwise backward error      eta_u = |r_u| / ((|G~ + lambda I|_F + a_u) |x_u| + |b_u|), 0 when the denominator is 0.
 * X is the block whose row u belongs to CSR row u (as in wmf_eval_sqerr); indptr may be a window into longer arrays (indices and
 * values are then the whole arrays).  dense is double [n, f], row-major without padding; NULL with out_rows == NULL (objective
 * only: no r / b work).  out_sums double[3], out_rows double[n, 3] or NULL, all on the device.
 * One wave per row; rows above 4096 entries get a workgroup each in a second launch.  No floating-point atomics and fixed
 * reduction orders: two runs give the same bits.
 * workspace: wmf_audit_workspace_bytes(n) bytes of device memory.  The calls only enqueue.  WMF_EINVAL, before any HIP call, for
 * a bad shape, a null pointer, out_rows without dense, or a workspace that is too small.
 * wmf_half_step_audit_f64: the same arithmetic on dense float64 factors X [n, f], Y [m, f] and float64 values -- the layouts of
 * wmf_half_step_f64. */
int64_t wmf_audit_workspace_bytes(int64_t n);
int wmf_half_step_audit(const float* X, const float* Y, int f, int ld, int bias,
                        const int64_t* indptr, const int32_t* indices, const float* values, int64_t n,
                        const double* dense, double* out_sums, double* out_rows,
                        void* workspace, int64_t workspace_bytes, void* stream);
int wmf_half_step_audit_f64(const double* X, const double* Y, int f, int bias,
                            const int64_t* indptr, const int32_t* indices, const double* values, int64_t n,
                            const double* dense, double* out_sums, double* out_rows,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* ---- why this item: the contributions of a row's stored entries to the scores of target items ------------------------------
 * For row u of a CSR (a user's history against the fixed side Y, the items) and a target item i, the score of i with the row
 * folded in -- predict with x_u = recompute_factors[_bias](Y, C_u, lambda), wmf_model.py:213-240 / :311-351 -- is a sum with one
 * term per stored entry.  With y~_j = row j of Y with column 0 read as 1 when bias != 0, beta_j = Y[j, 0] when bias != 0, else 0,
 * w_e = c_e - beta_j for the stored entry e = (j, c_e) (wmf_model.py:343), and A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T, x_u =
 * A_u^-1 sum_e (w_e + 1) y~_j of wmf_model.py:231-239 and :343-350:
 *     contrib(u, i, e) = (w_e + 1) y~_i^T A_u^-1 y~_j,        total(u, i) = sum_e contrib(u, i, e) + beta_i = y~_i . x_u + beta_i.
 * With a bias model the row's own bias x_u[0] is part of x_u and so is shared out over the entries.  The row is read as stored:
 * stored zeros count, duplicates are separate entries.  Solved in whitened coordinates q = y~ W_white, where A_u becomes
 * I + E_u, E_u = sum_e w_e q_j q_j^T, with a condition number of at most 1 + max w: float32 Cholesky, one workgroup per row, the
 * row's system in LDS at every width f = 1 .. WMF_MAX_F.
 * Inputs: all arrays on the device.  Y [m, ld] is the UN-whitened fixed side in the library's layout, W_white [f, ld] what
 *   wmf_factorize returns for wmf_gram(Y, bias) and lambda (upper triangular: the entries below the diagonal are not read).
 *   The kernel whitens what it gathers; no whitened copy of Y is made or needed.  indptr is int64[n + 1] and may be a window into
 *   longer arrays (indices and values are then the whole arrays); values are confidences.  targets is int32 [n, n_targets]: item
 *   ids in [0, m), or -1 for an empty slot; an item may occur several times in a row (its columns then hold the same bits).
 * Outputs: out_contrib[p * n_targets + t] = the contribution of the stored entry at absolute position p to target t of its row
 *   (the pointer indexes like indices).  out_total [n, n_targets] = the row's contributions added one by one in stored order in
 *   float32, starting from 0, and then + beta_i; an empty row gives beta_i.  A -1 slot writes 0 to every output of that slot.
 *   Every output element is written.
 * Failures: a row whose I + E_u is not positive definite (a pivot <= 0 or not finite: only possible with effective weights <= -1)
 *   gets NaN in every contribution and total of its non-empty slots and is counted once in fail_count (device int32, the caller
 *   zeroes it, as for wmf_solve_rows).
 * Limits: 1 <= n_targets <= WMF_EXPLAIN_MAX_TARGETS (split longer lists; WMF.explain does), 1 <= m < 2^31, 0 <= n < 2^31; n == 0
 *   is a no-op.  workspace: wmf_explain_workspace_bytes(n, f, n_targets) bytes of device memory (a small constant: reserved, not
 *   written -- every width fits LDS).
 * The call only enqueues.  WMF_EINVAL, before any HIP call, for a bad shape, a null pointer, n_targets out of range or a workspace
 * that is too small.  No floating-point atomics and fixed reduction orders: two runs give the same bits, a row's outputs do not
 * depend on the other rows of the launch, a target's column does not depend on the other targets of its row. */
#define WMF_EXPLAIN_MAX_TARGETS 16
int64_t wmf_explain_workspace_bytes(int64_t n, int f, int32_t n_targets);
int wmf_explain_rows(const float* Y, int64_t m, int f, int ld, int bias, const float* W_white,
                     const int64_t* indptr, const int32_t* indices, const float* values, int64_t n,
                     const int32_t* targets, int32_t n_targets,
                     float* out_contrib, float* out_total, int32_t* fail_count,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* ---- fold a history in: the factors of rows that were never trained on -----------------------------------------------------
 * For row u of a CSR (a history against the fixed side Y, the items) the row a user half step would give it:
 *     X_out[u] = x_u = A_u^-1 sum_e (w_e + 1) y~_j,        A_u = G~ + lambda I + sum_e w_e y~_j y~_j^T
 * over the stored entries e = (j, c_e) of the row, with y~_j, beta_j and w_e = c_e - beta_j as defined for wmf_explain_rows: row u
 * of recompute_factors[_bias](Y, C, lambda), wmf_model.py:213-240 / :311-351 (the row system of :231-239 / :343-350).  It is the
 * x_u of wmf_explain_rows: y~_i . x_u + beta_i is that call's total(u, i).  The row is read as stored: stored zeros count,
 * duplicates are separate entries.  Solved in whitened coordinates q = y~ W_white: (I + E_u) g = b with E_u = sum_e w_e q_j q_j^T
 * and b = sum_e (w_e + 1) q_j, x_u = W_white g; float32 Cholesky, one workgroup per row, the row's system in LDS at every width
 * f = 1 .. WMF_MAX_F.
 * Inputs: those of wmf_explain_rows -- all arrays on the device, Y [m, ld] the UN-whitened fixed side in the library's layout,
 *   W_white [f, ld] what wmf_factorize returns for wmf_gram(Y, bias) and lambda (the entries below the diagonal are not read),
 *   indptr int64[n + 1], possibly a window into longer indices / values arrays; values are confidences.
 * Output: X_out [n, ld] in the library's layout: row u is a row of `users` -- with bias != 0 column 0 is the row's own bias, as in
 *   the output of recompute_factors_bias -- and the padding columns [f, ld) are written as zeros, so the block can be handed to
 *   wmf_recommend_topn, wmf_predict_pairs or wmf_similar_topn as it is.  An empty row gives zeros (wmf_model.py:274-276).  Every
 *   element of the n rows is written.
 * Failures: a row whose I + E_u is not positive definite (a pivot <= 0 or not finite: only possible with effective weights <= -1)
 *   gets NaN in its f columns (zeros in its padding) and is counted once in fail_count (device int32, the caller zeroes it).
 * Limits: 1 <= m < 2^31, 0 <= n < 2^31; n == 0 is a no-op.  workspace: wmf_foldin_workspace_bytes(n, f) bytes of device memory
 *   (a small constant: reserved, not written -- every width fits LDS).
 * The call only enqueues.  WMF_EINVAL, before any HIP call, for a bad shape, a null pointer or a workspace that is too small.  No
 * floating-point atomics and fixed reduction orders: two runs give the same bits, a row's output does not depend on the other
 * rows of the launch or on its position in it. */
int64_t wmf_foldin_workspace_bytes(int64_t n, int f);
int wmf_foldin_rows(const float* Y, int64_t m, int f, int ld, int bias, const float* W_white,
                    const int64_t* indptr, const int32_t* indices, const float* values, int64_t n,
                    float* X_out, int32_t* fail_count,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the posterior of a folded-in row: Thompson draws, and the mean and variance of a score ----------------------------------
 * The probabilistic reading of the row system of wmf_foldin_rows: a Gaussian likelihood with precision w_e + 1 on a stored entry and
 * 1 on every other item, a Gaussian prior of precision lambda and unit noise give the row the posterior N(x_u, A_u^-1) -- x_u and
 * A_u as defined there.  In whitened coordinates q = y~ W_white, with I + E_u = L L^T (float32 Cholesky), b = sum_e (w_e + 1) q_j and
 * c = L^-1 b:  A_u^-1 = W_white L^-T L^-1 W_white^T, because W_white W_white^T = (G~ + lambda I)^-1.
 *
 * wmf_posterior_draw_rows: n_draws draws of every row,
 *     X_out[u * n_draws + s] = x~_s = W_white L^-T (c + sigma xi_s),      xi_s: f standard normal variates,
 *   with mean x_u and covariance sigma^2 A_u^-1.  The right-hand side is fmaf(sigma, xi, c), component by component; sigma == 0 takes c
 *   itself (no product), and the result is then wmf_foldin_rows's, bit for bit, in every one of the n_draws rows.
 *   The noise is a pure function of (seed, stream, draw, component) -- no generator with state (mix: see wmf_sample_topn):
 *     a  = mix(seed + 0x9E3779B97F4A7C15 * (stream + 1))             the row prefix of wmf_sample_topn
 *     h  = mix(a + 0x9E3779B97F4A7C15 * (2^32 * (draw + 1) + component + 1))
 *     k1 = h >> 41;  k2 = (h >> 18) & 0x7FFFFF                       23 bits each
 *     u1 = (2 k1 + 1) * 2^-24;  t = (2 k2 + 1) * 2^-23               both exact in float32
 *     xi = sqrtf(-2 logf(u1)) * cospif(t)                            the accurate functions
 *   stream: row_stream[u], a uint64 per row on the device; row_stream == NULL: stream = u.  The keys are at least 2^32 + 1, those of
 *   wmf_sample_topn's items at most 2^32: one (seed, stream) serves both without a shared hash input.  The tail is cut off:
 *   |xi| <= sqrt(48 ln 2) = 5.768 (a variate beyond it, probability 8e-9, is never drawn).  Draw s has the same bits whatever n_draws
 *   is, whatever the row's position and whatever the other rows of the launch are.
 *   X_out is [n * n_draws, ld] in the library's layout, the padding columns written as zeros: a block of rows of `users` for
 *   wmf_recommend_topn*.  An EMPTY row has I + E_u = I and c = 0: its draws are the prior's, W_white sigma xi_s (zeros at sigma == 0,
 *   as wmf_foldin_rows).  Limits: 1 <= n_draws <= WMF_POSTERIOR_MAX_DRAWS, n * n_draws < 2^31, sigma finite and >= 0.
 *
 * wmf_posterior_score_rows: for targets int32 [n, n_targets] (item ids in [0, m), -1 for an empty slot), with z_i = L^-1 q_i,
 *     out_var[u, t]  = z_i . z_i          = y~_i^T A_u^-1 y~_i: the variance of the score, a sum of squares and so never negative;
 *     out_mean[u, t] = z_i . c + beta_i   = y~_i . x_u + beta_i in exact arithmetic: wmf_explain_rows's total, predict on the folded-in row.
 *   An empty row gives var = |q_i|^2, the prior variance, and mean = beta_i.  A -1 slot writes 0 to both.  Either output may be NULL,
 *   not both.  A target's outputs do not depend on the other targets of its row.  Limits: 1 <= n_targets <=
 *   WMF_POSTERIOR_MAX_TARGETS (split longer lists; WMF.score_posterior does).
 *
 * Both: the inputs of wmf_foldin_rows (all arrays on the device, Y un-whitened, indptr possibly a window; 1 <= m < 2^31, 0 <= n <
 *   2^31, n == 0 a no-op).  One 256-thread workgroup per row, the row's system in LDS at every width f = 1 .. WMF_MAX_F; the gather and
 *   the factorisation are wmf_foldin_rows's, operation for operation; then 16 right-hand sides at a time, a 16-lane group each.  A row
 *   whose I + E_u is not positive definite gets NaN in the f columns of all its draws (zeros in the padding), or in both outputs of
 *   its non-empty slots, and is counted once in fail_count (device int32, the caller zeroes it).  Every output element is written.
 *   workspace: wmf_posterior_{draw,score}_workspace_bytes (a small constant: reserved, not written).  The call only enqueues.
 *   WMF_EINVAL, before any HIP call and with the outputs untouched, for a bad shape, a null pointer (row_stream and one score output
 *   excepted), a count out of range, n * n_draws >= 2^31, a sigma that is negative or not finite, or a workspace that is too small.
 *   No floating-point atomics and fixed reduction orders: two runs give the same bits; a row's outputs depend on nothing but the row
 *   and, for the draws, its stream.
 * wmf_posterior_noise: xi (out_xi, may be NULL) and k1, k2 (out_k1k2 uint32 [n, 2], may be NULL) of n arbitrary (row_stream[i],
 *   draws[i], components[i]) triples from the draw kernel's own device function (row_stream == NULL: stream = i; draws and components
 *   int32 in [0, 2^31)): what the exact tests stand on.  WMF_EINVAL for n < 0, a null draws or components, or both outputs null.
 * Measured (MI355X, 2048 rows, 1 000 000 items, k = 128 + biases, about 10 / 100 entries per row; profiles/r26_posterior.json): one draw
 *   per row 1.15 / 2.35 ms where wmf_foldin_rows takes 1.15 / 2.53 ms, 16 draws 1.26 / 2.44 ms; 100 targets per row 3.5 / 4.7 ms, 1000
 *   targets 24.6 / 25.7 ms (a pass of 16 targets costs a whitening and f barriers: torch's batched float64 Cholesky route is the
 *   faster one for the variances of many targets, 4.05 / 4.61 ms for the mean, 16 draws and 100 variances). */
#define WMF_POSTERIOR_MAX_DRAWS 4096
#define WMF_POSTERIOR_MAX_TARGETS 4096
int64_t wmf_posterior_draw_workspace_bytes(int64_t n, int f, int32_t n_draws);
int wmf_posterior_draw_rows(const float* Y, int64_t m, int f, int ld, int bias, const float* W_white,
                            const int64_t* indptr, const int32_t* indices, const float* values, int64_t n,
                            int32_t n_draws, float sigma, uint64_t seed, const uint64_t* row_stream,
                            float* X_out, int32_t* fail_count,
                            void* workspace, int64_t workspace_bytes, void* stream);
int64_t wmf_posterior_score_workspace_bytes(int64_t n, int f, int32_t n_targets);
int wmf_posterior_score_rows(const float* Y, int64_t m, int f, int ld, int bias, const float* W_white,
                             const int64_t* indptr, const int32_t* indices, const float* values, int64_t n,
                             const int32_t* targets, int32_t n_targets,
                             float* out_mean, float* out_var, int32_t* fail_count,
                             void* workspace, int64_t workspace_bytes, void* stream);
int wmf_posterior_noise(uint64_t seed, const uint64_t* row_stream, const int32_t* draws, const int32_t* components, int64_t n,
                        float* out_xi, uint32_t* out_k1k2, void* stream);

/* out[p] = predict(users_idx[p], items_idx[p])   wmf_model.py:205-211.
 * n_u == 1 or n_i == 1 broadcasts that index (the reference's one-user / one-item form).
 * An empty side (n_u == 0 or n_i == 0, the other 0 or 1) has no pairs: WMF_OK, nothing is read or written. */
int wmf_predict_pairs(const float* users, const float* items, int f, int ld, int bias,
                      const int32_t* users_idx, int64_t n_u, const int32_t* items_idx, int64_t n_i,
                      float* out, void* stream);

/* WMF.rank, wmf_model.py:25-47: scores of ONE user (*user_idx, device) against n_cand candidate item rows
 * (cand_idx, device), the topn best sorted by score, best first.  out_pos[k] = position in cand_idx of the k-th best
 * candidate (the reference returns items[order]); ties keep candidate order (the reference's tie order is
 * whatever argpartition / argsort leave).  out_scores may be NULL.  1 <= topn <= n_cand.
 * A top-n select like the reference's argpartition (:40-43), not a sort of all candidates: only the candidates of the
 * score-histogram bins that reach down to the topn-th best are sorted.  The length of that list is read back, so this
 * call SYNCHRONISES its stream.  workspace: wmf_rank_workspace_bytes(n_cand) bytes of device memory. */
int64_t wmf_rank_workspace_bytes(int64_t n_cand);
int wmf_rank_topn(const float* users, const float* items, int f, int ld, int bias, const int32_t* user_idx,
                  const int32_t* cand_idx, int64_t n_cand, int64_t topn, int32_t* out_pos, float* out_scores,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* WMF.rank with a LIST of users (wmf_model.py:29-32 loops; here one launch): every user in user_idx (n_users,
 * device) against the same candidate list; out_pos[u * topn + k] = position in cand_idx of user u's k-th best.
 * Scores by f32 MFMA (16 users x 16 candidates per wave), ordering by a stable segmented radix sort.
 * n_users * n_cand < 2^31; workspace: wmf_rank_batch_workspace_bytes(n_users, n_cand). */
int64_t wmf_rank_batch_workspace_bytes(int64_t n_users, int64_t n_cand);
int wmf_rank_topn_batch(const float* users, const float* items, int f, int ld, int bias, const int32_t* user_idx,
                        int64_t n_users, const int32_t* cand_idx, int64_t n_cand, int64_t topn, int32_t* out_pos,
                        float* out_scores, void* workspace, int64_t workspace_bytes, void* stream);

/* The topn best items of the WHOLE catalogue [0, n_items) for every user of a batch, leaving out the items the user has
 * seen: what RecModel/utils.py:3-17 (test_coverage) asks of WMF.rank (wmf_model.py:25-47) with
 * np.delete(arange(n_items), seen) as the candidates, for all users in one fused pass -- scores by f32 MFMA, a running
 * top-n per user; nothing of size n_users x n_items is ever stored.
 * Inputs: all arrays on the device, factors in the library's layout (ld % 4 == 0, zero padding).  user_idx[b] selects the
 *   user row of batch position b; a user may occur several times.
 * Seen list: seen_indptr is int64[n_users + 1]; row b of that CSR belongs to batch position b (not to the user id);
 *   seen_indices are item ids in [0, n_items), ascending within a row, duplicates allowed; the CSR is read as stored.
 *   seen_indptr == NULL: nothing is excluded.
 * Order: a higher score wins, equal scores go to the lower item id (-0.0 and +0.0 are equal).
 * Outputs: out_items[b * topn + k] = the k-th best item not in row b.  out_scores (may be NULL) = its score, the same
 *   arithmetic as wmf_rank_topn_batch (bit for bit) and wmf_predict_pairs.  out_count[b] (may be NULL) = min(topn, eligible
 *   items); entries past it hold item -1 and score -inf.
 * Limits: 1 <= topn <= WMF_RECOMMEND_MAX_TOPN, n_users >= 1, 1 <= n_items < 2^31.
 * Slices: the catalogue is scanned in n_slices contiguous slices whose partial results are merged, so that a handful of
 *   users still fills the device; the result does not depend on n_slices.  0: the library chooses from n_users, n_items and
 *   the device's CU count, at most WMF_RECOMMEND_AUTO_SLICES; 1 .. WMF_RECOMMEND_MAX_SLICES forces it (slices beyond the
 *   number of 16-item tiles are empty).
 * Workspace: wmf_recommend_workspace_bytes(n_users, topn, n_slices) bytes of device memory =
 *   WMF_RECOMMEND_WS_BASE + WMF_RECOMMEND_WS_PER_KEY * n_users * topn * (n_slices, or WMF_RECOMMEND_AUTO_SLICES for 0):
 *   it does not depend on n_items.
 * The call only enqueues: it does not allocate, synchronise or read back (unlike wmf_rank_topn).  WMF_EINVAL, before any
 * HIP call, for a bad shape, a null pointer, topn or n_slices out of range or a workspace that is too small.
 * Factors are finite; infinite scores order as floats; NaN scores are unspecified, but every index written is in range. */
#define WMF_RECOMMEND_MAX_TOPN 128
#define WMF_RECOMMEND_MAX_SLICES 256
#define WMF_RECOMMEND_AUTO_SLICES 64
#define WMF_RECOMMEND_WS_BASE 256
#define WMF_RECOMMEND_WS_PER_KEY 8
int64_t wmf_recommend_workspace_bytes(int64_t n_users, int64_t topn, int32_t n_slices);
int wmf_recommend_topn(const float* users, const float* items, int f, int ld, int bias,
                       const int32_t* user_idx, int64_t n_users, int64_t n_items,
                       const int64_t* seen_indptr, const int32_t* seen_indices,
                       int64_t topn, int32_t n_slices,
                       int32_t* out_items, float* out_scores, int32_t* out_count,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* wmf_recommend_topn over a PART of the catalogue: what is in stock, licensed, on a shelf.  The same fused scan, the same seen
 * list, order, outputs, padding, limits, slices and workspace (wmf_recommend_workspace_bytes); out_count[b] = min(topn, eligible
 * items not seen).  The part is given in one of two forms, all arrays on the device:
 * Mask form: allow_bits is uint32[n_masks][allow_words], allow_words >= ceil(n_items / 32), n_masks >= 1.  Item j is eligible under
 *   mask g exactly when bit j & 31 of word j >> 5 of row g is set; bits of j >= n_items are ignored.  allow_idx is int32[n_users]
 *   with values in [-1, n_masks): the mask of batch position b; NULL: every position uses mask 0; -1: that position is unrestricted.
 *   Values outside the range are the caller's error.  The whole catalogue is scored; the bit is tested where an item would be
 *   inserted, after the threshold and before the seen list, so the cost over wmf_recommend_topn is that of the insertions a low pass
 *   rate adds (the threshold rises more slowly).
 * List form: cand_idx is int32[n_cand], strictly ascending item ids in [0, n_items), 1 <= n_cand <= n_items (a precondition, like
 *   the order of the seen list).  Only those rows are read and scored, in 16-position tiles; slices are cut from the n_cand
 *   positions; the cost is proportional to n_cand.  Keys, seen lookups and outputs use the item ids, not the positions.
 * One form per call: both is WMF_EINVAL; neither is wmf_recommend_topn, bit for bit (the same kernels).  allow_bits with
 *   n_masks < 1 or allow_words too small, allow_idx without allow_bits, cand_idx with n_cand outside [1, n_items]: WMF_EINVAL.
 *   All refusals come before any HIP call.
 * A score is one lane's element of a 16 x 16 MFMA tile summed over the features in a fixed order: it does not depend on the tile
 * position an item has.  So both forms return, bit for bit, the items and scores that wmf_recommend_topn returns when the ineligible
 * items are appended to every row's seen list; the result does not depend on n_slices.  The call only enqueues.
 * Measured (MI355X, 2048 users x 1 000 000 items, k = 128 + biases, topn 10; profiles/r19_recommend_filtered.json): the mask form's
 * scan takes -4 .. +4.5 % of the unfiltered scan's 10.3 ms at pass rates from 50 % to 0.01 %; the list form's 0.15 ms for 99 ids,
 * 0.54 ms for 10 000, 6.3 ms for 500 000 and 11.7 ms for all 1 000 000 (the gather costs 14 % at full length): by the kernels the
 * forms cross near 870 000 ids, by the whole Python call, which also sorts and uploads the ids, near 575 000. */
int wmf_recommend_topn_filtered(const float* users, const float* items, int f, int ld, int bias,
                                const int32_t* user_idx, int64_t n_users, int64_t n_items,
                                const int64_t* seen_indptr, const int32_t* seen_indices,
                                const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks, const int32_t* allow_idx,
                                const int32_t* cand_idx, int64_t n_cand,
                                int64_t topn, int32_t n_slices,
                                int32_t* out_items, float* out_scores, int32_t* out_count,
                                void* workspace, int64_t workspace_bytes, void* stream);

/* wmf_recommend_topn_filtered for 1 <= topn <= WMF_RECOMMEND_WIDE_MAX_TOPN: the candidate pool of a two-stage recommender, the
 * lists behind Recall@500.  The contract of wmf_recommend_topn_filtered in every respect but the limit: the same arguments, seen
 * list per batch position, order (a higher score wins, equal scores go to the lower id, -0.0 equals +0.0), out_count, -1 / -inf
 * padding; the call only enqueues, and every refusal (WMF_EINVAL) comes before any HIP call and leaves the outputs untouched.
 * Filter forms: neither allow_bits nor cand_idx is an unfiltered call; exactly one of them is a filtered call (the mask form, the
 *   list form); both is WMF_EINVAL, as are n_masks < 1, allow_words too small, allow_idx without allow_bits and n_cand outside
 *   [1, n_items].
 * Kernels: every topn from 1 to the limit runs the wide kernels -- nothing routes a small topn to wmf_recommend_topn's.  The scan
 *   and its arithmetic are those of wmf_recommend_topn (the scores are the same bits); a row's running keys live in the workspace
 *   instead of LDS, one buffer of WMF_RECOMMEND_WIDE_CAP(topn) keys per (batch position, slice), cut back to its topn best by an
 *   exact radix select whenever the next tile could overflow it; a selection kernel then takes the topn best of a row's slices and
 *   sorts them.  For topn <= WMF_RECOMMEND_MAX_TOPN the result equals wmf_recommend_topn[_filtered]'s bit for bit.
 * Slices: 0: the library chooses; 1 .. WMF_RECOMMEND_MAX_SLICES forces it; the result does not depend on it.  The automatic count
 *   is S0 = L0 / n_users (rounded down), L0 = min(WMF_RECOMMEND_WIDE_AUTO_SLICES * n_users, max(WMF_RECOMMEND_WIDE_AUTO_LISTS,
 *   n_users)) lists -- 512 workgroups of 64 rows, enough to fill the device, at most WMF_RECOMMEND_WIDE_AUTO_SLICES slices --
 *   lowered until a slice holds at least max(1024, WMF_RECOMMEND_WIDE_SLICE_TOPNS * topn) of the scanned positions (n_items, or
 *   n_cand in the list form): a row inserts about topn (1 + ln(slice / topn)) keys per slice, each a seen-list search and a global
 *   store, and they stay rare only while a slice is several times longer than topn.
 * Workspace: wmf_recommend_wide_workspace_bytes(n_users, topn, n_slices) = WMF_RECOMMEND_WIDE_WS_BASE + L *
 *   (WMF_RECOMMEND_WIDE_WS_PER_KEY * WMF_RECOMMEND_WIDE_CAP(topn) + WMF_RECOMMEND_WIDE_WS_PER_LIST), L = n_users * n_slices lists,
 *   or L0 above for n_slices = 0.  Pure host code; it does not depend on n_items and grows with each of its arguments.
 * Measured (MI355X, 1 000 000 items, k = 128 + biases, 10 seen items per row; profiles/r20_recommend_wide.json): 16 users at topn
 *   200 in 5.2 ms where the host loop of WMF.recommend took 111 ms; 2048 users in 17.9 / 21.8 / 27.6 / 36.7 ms at topn 129 / 256 /
 *   512 / 1000 (scan 17.0 .. 33.3 ms, selection 0.16 .. 0.90 ms), 16 users in 4.4 .. 16.7 ms at topn 129 .. 4096; at topn 128 the
 *   scan takes 17.1 ms where wmf_recommend_topn's two-wave scan takes 46.9; the mask form at a 1 % pass rate 14.9 ms and the list
 *   form of 10 000 ids 6.0 ms at topn 1000.  At topn 2048 / 4096 a row needs 4 / 2 MB of workspace at 62 / 31 slices: force fewer
 *   slices, or call with fewer rows, when that is too much. */
#define WMF_RECOMMEND_WIDE_MAX_TOPN 4096
#define WMF_RECOMMEND_WIDE_AUTO_SLICES 64
#define WMF_RECOMMEND_WIDE_AUTO_LISTS 32768
#define WMF_RECOMMEND_WIDE_SLICE_TOPNS 8
#define WMF_RECOMMEND_WIDE_CAP(topn) (2 * (topn) > 32 ? 2 * (topn) : 32)
#define WMF_RECOMMEND_WIDE_WS_BASE 256
#define WMF_RECOMMEND_WIDE_WS_PER_KEY 8
#define WMF_RECOMMEND_WIDE_WS_PER_LIST 8
int64_t wmf_recommend_wide_workspace_bytes(int64_t n_users, int64_t topn, int32_t n_slices);
int wmf_recommend_topn_wide(const float* users, const float* items, int f, int ld, int bias,
                            const int32_t* user_idx, int64_t n_users, int64_t n_items,
                            const int64_t* seen_indptr, const int32_t* seen_indices,
                            const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks, const int32_t* allow_idx,
                            const int32_t* cand_idx, int64_t n_cand,
                            int64_t topn, int32_t n_slices,
                            int32_t* out_items, float* out_scores, int32_t* out_count,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* SAMPLED top-n: n items per row drawn WITHOUT replacement from softmax(score / temperature) over the row's eligible items -- a
 * Plackett-Luce draw -- in one scan of the catalogue, for exploration slates, hard negatives in proportion to the model's own
 * softmax, and the propensities of off-policy evaluation (wmf_log_partition).  The Gumbel-top-n identity: the n largest of
 * z_i = score_i + temperature * g_i, g_i i.i.d. standard Gumbel, are such a draw, in draw order.
 * The noise is a pure function of (seed, stream, item) -- no generator with state -- so a row's list does not depend on its batch
 *   position, the other rows, the slice count, the grid or the form of the filter:
 *     mix(z):  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31      (uint64, wrapping)
 *     a = mix(seed + 0x9E3779B97F4A7C15 * (stream + 1))             once per row
 *     h = mix(a    + 0x9E3779B97F4A7C15 * (item   + 1))             item zero-extended from its 32-bit id
 *     k = h >> 41                                                   23 bits
 *     u = (2 k + 1) * 2^-24                                         exact in float32, in [2^-24, 1 - 2^-24]
 *     g = -logf(-logf(u))                                           the accurate logf
 *   stream: row_stream[b], a uint64 per batch position on the device; row_stream == NULL: stream = b.
 * The tail is cut off: g lies in [-2.8116, 16.6356] and is never above WMF_SAMPLE_G_MAX, the float32 value of g at k = 2^23 - 1;
 *   relative probabilities below about e^-16 are not resolved (an item 17 / temperature below the row's best is never drawn first).
 * Contract: that of wmf_recommend_topn_wide in every respect except the order -- the arguments, the three filter forms, 1 <= n <=
 *   WMF_RECOMMEND_WIDE_MAX_TOPN, the -1 / -inf padding, out_count, the slice rules and the workspace formula
 *   (wmf_sample_workspace_bytes = wmf_recommend_wide_workspace_bytes); the call only enqueues, and every refusal (WMF_EINVAL) comes
 *   before any HIP call and leaves the outputs untouched.
 * Order: by z = fmaf(temperature, g, score), largest first; equal z goes to the lower id, -0.0 equals +0.0.  In the list form the
 *   noise is keyed by the item's id, not by its place in the list.
 * Outputs: out_items; out_scores (may be NULL): the MODEL's score of each pick, the bits wmf_recommend_topn_wide returns for that
 *   item; out_keys (may be NULL): z; out_count (may be NULL).
 * temperature: finite and >= 0 (WMF_EINVAL otherwise).  temperature == 0: z = score, and the result is wmf_recommend_topn_wide's bit
 *   for bit, from these kernels, for any seed.
 * wmf_sample_noise: g (out_g, may be NULL) and k (out_k, may be NULL) of n_pairs arbitrary (row_stream[i], items[i]) pairs from the
 *   scan's own device function (row_stream == NULL: stream = i): what the exact tests stand on.  WMF_EINVAL for n_pairs < 0, a null
 *   items or both outputs null.
 * Measured (MI355X, 1 000 000 items, k = 128 + biases, 10 seen items per row; profiles/r25_sample.json): 2048 rows at n = 10 / 100 /
 *   1000 in 15.0 / 19.3 / 36.7 ms at temperature 1 and 13.1 / 17.9 / 36.8 ms at temperature 0, where wmf_recommend_topn_wide takes
 *   12.2 / 16.2 / 34.0 ms: 1.08 to 1.24 x, with the WMF_SAMPLE_G_MAX skip in; wmf_log_partition of 2048 rows 19.1 ms. */
#define WMF_SAMPLE_G_MAX 0x1.0a2b24p+4f
int64_t wmf_sample_workspace_bytes(int64_t n_rows, int64_t n, int32_t n_slices);
int wmf_sample_topn(const float* users, const float* items, int f, int ld, int bias,
                    const int32_t* user_idx, int64_t n_rows, int64_t n_items,
                    const int64_t* seen_indptr, const int32_t* seen_indices,
                    const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks, const int32_t* allow_idx,
                    const int32_t* cand_idx, int64_t n_cand,
                    int64_t n, int32_t n_slices, float temperature, uint64_t seed, const uint64_t* row_stream,
                    int32_t* out_items, float* out_scores, float* out_keys, int32_t* out_count,
                    void* workspace, int64_t workspace_bytes, void* stream);
int wmf_sample_noise(uint64_t seed, const uint64_t* row_stream, const int32_t* items, int64_t n_pairs,
                     float* out_g, uint32_t* out_k, void* stream);

/* log Z[b] = log sum exp(score / temperature) over the items row b may see: with it, score / temperature - log Z is the log of the
 * probability with which wmf_sample_topn draws an item FIRST under the same filter.  The rows, the three filter forms and the
 * slice arguments of wmf_recommend_topn_wide; temperature finite and > 0.  out_logz: float32 per row; out_eligible (may be NULL):
 * the number of eligible items, exactly.  A row with nothing eligible gets -inf and 0.
 * Kernels: one scan with a log-sum-exp epilogue -- a running (max, sum) per lane, the max in float32, a term expf((s - max) /
 *   temperature) in float32, the sum in float64, a lane's partial per (row, slice) in the workspace -- and a merge that combines a
 *   row's partials in a fixed order in float64 and rounds once.  No floating-point atomics: two runs at one slice count are
 *   bit-identical; other slice counts agree within the error below.
 * Error: against the float64 log-sum-exp of float64 scores, |L - L64| <= B / temperature + 4 * 2^-23 * (2 + ln n_eligible) + 2^-23 *
 *   |L64|, B the float32 score's own error bound: a term's relative error is 2^-23 (1 + |x|), x = (s - max) / temperature, the
 *   softmax mean of |x| is at most ln n_eligible, and the factor 4 covers the rescales of the running max.
 * Workspace: wmf_log_partition_workspace_bytes(n_rows, n_slices) = WMF_RECOMMEND_WIDE_WS_BASE + L * 16 *
 *   WMF_LOG_PARTITION_WS_PER_LANE, L the lists of wmf_recommend_wide_workspace_bytes; the automatic slices are those of
 *   wmf_recommend_topn_wide at topn 1.  WMF_EINVAL, before any HIP call and with the outputs untouched, as wmf_recommend_topn_wide. */
#define WMF_LOG_PARTITION_WS_PER_LANE 16
int64_t wmf_log_partition_workspace_bytes(int64_t n_rows, int32_t n_slices);
int wmf_log_partition(const float* users, const float* items, int f, int ld, int bias,
                      const int32_t* user_idx, int64_t n_rows, int64_t n_items,
                      const int64_t* seen_indptr, const int32_t* seen_indices,
                      const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks, const int32_t* allow_idx,
                      const int32_t* cand_idx, int64_t n_cand,
                      float temperature, int32_t n_slices, float* out_logz, int32_t* out_eligible,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* One list per (row, GROUP) from ONE scan of the catalogue: the topn best items of each of n_groups shelves (genres, departments,
 * carousels) for every row of a batch.  group_of is int32[n_items] on the device: item j is on shelf group_of[j]; any value outside
 * [0, n_groups) -- -1, for instance -- means "on no shelf", and the item is never returned (the test is unsigned: every index
 * derived from the value is in range whatever the caller passes).
 * Contract: list (b, g) is, bit for bit (items, score bits, count, padding), what wmf_recommend_topn_filtered returns for row b under
 *   the mask {j : group_of[j] == g}, intersected with the row's allow mask if any; equivalently, wmf_recommend_topn with the
 *   complement appended to the row's seen list.  The seen list, order (a higher score wins, equal scores go to the lower id, -0.0
 *   equals +0.0) and -1 / -inf padding are those of wmf_recommend_topn.
 * Outputs: out_items[(b * n_groups + g) * topn + k], out_scores (may be NULL) likewise, out_count[b * n_groups + g] (may be NULL) =
 *   min(topn, eligible unseen items of the group).
 * Filter: the mask form of wmf_recommend_topn_filtered (allow_bits, allow_words, n_masks, allow_idx), or allow_bits == NULL for
 *   none.  There is no list form.
 * Limits: 1 <= n_groups <= WMF_RECOMMEND_GROUPS_MAX, 1 <= topn <= WMF_RECOMMEND_MAX_TOPN (shelves are short), otherwise those of
 *   wmf_recommend_topn_wide.
 * Kernels: the scan, arithmetic and keys of wmf_recommend_topn_wide (the scores are the same bits), every score computed once; a
 *   row's running keys live in the workspace, one buffer of WMF_RECOMMEND_WIDE_CAP(topn) keys per (row, group, slice), thresholds
 *   and counts of a wave's 16 x n_groups buffers in LDS (768 bytes per group and workgroup); wmf_recommend_topn_wide's selection
 *   kernel then finishes the n_users * n_groups lists.
 * Slices: 0: the automatic count of wmf_recommend_topn_wide with topn * n_groups in place of topn for the minimum slice length (with
 *   even groups a slice then holds at least WMF_RECOMMEND_WIDE_SLICE_TOPNS x topn items of every group; uneven groups cost
 *   insertions, never correctness); 1 .. WMF_RECOMMEND_MAX_SLICES forces it.  The result does not depend on it.
 * Workspace: wmf_recommend_grouped_workspace_bytes(n_users, n_groups, topn, n_slices) = WMF_RECOMMEND_WIDE_WS_BASE + n_groups * L *
 *   (WMF_RECOMMEND_WIDE_WS_PER_KEY * WMF_RECOMMEND_WIDE_CAP(topn) + WMF_RECOMMEND_WIDE_WS_PER_LIST), L the list count of
 *   wmf_recommend_wide_workspace_bytes for the same n_users and n_slices.  Pure host code; it does not depend on n_items and grows
 *   with each of its arguments.
 * The call only enqueues.  WMF_EINVAL, before any HIP call and with the outputs untouched, for a null group_of, users, items,
 *   user_idx, out_items or workspace, n_groups, topn or n_slices out of range, a workspace that is too small, and the mask-argument
 *   refusals of wmf_recommend_topn_filtered.
 * Measured (MI355X, 1 000 000 items, k = 128 + biases, 10 seen items per row, topn 10, shelves j mod G, whole Python calls;
 *   profiles/r22_recommend_shelves.json): 2048 users x 16 shelves in 40.8 ms (scan 37.4, selection 1.4) where
 *   wmf_recommend_topn_filtered with every user repeated 16 times under 16 masks takes 160.8 ms, the arrays identical; 21.7 against
 *   40.1 ms at 4 shelves, 17.1 against 19.7 at 2, 151 ms at 64 (the repeated rows: 91 ms for 256 of the users).  Over one unfiltered
 *   wide scan (12.8 ms) that is 1.15 x at one shelf, 1.7 x at 4, 3.2 x at 16 and 11.8 x at 64: the insertions and cuts of G buffers a
 *   row.  The repeated rows win at one shelf (10.8 against 14.3 ms) and for a handful of rows (16 users x 16 shelves: 5.0 against
 *   14.1 ms). */
#define WMF_RECOMMEND_GROUPS_MAX 64
int64_t wmf_recommend_grouped_workspace_bytes(int64_t n_users, int32_t n_groups, int64_t topn, int32_t n_slices);
int wmf_recommend_topn_grouped(const float* users, const float* items, int f, int ld, int bias,
                               const int32_t* user_idx, int64_t n_users, int64_t n_items,
                               const int64_t* seen_indptr, const int32_t* seen_indices,
                               const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks, const int32_t* allow_idx,
                               const int32_t* group_of, int32_t n_groups,
                               int64_t topn, int32_t n_slices,
                               int32_t* out_items, float* out_scores, int32_t* out_count,
                               void* workspace, int64_t workspace_bytes, void* stream);

/* Inverse row norms over the FEATURE columns, the scales of a cosine (wmf_similar_topn):
 * out[i] = 1 / sqrt(S_i) rounded to float32, S_i = sum over the columns c in [bias, f) of M[i, c]^2 accumulated in float64 in a
 * fixed order (two calls give the same bits); 0 where S_i == 0 or the quotient is not a finite float32.  With bias != 0 column 0
 * is the bias and no feature; the padding columns [f, ld) are not read as features.  M is [n, ld] in the library's layout, out
 * float32[n], both on the device; n == 0 is a no-op.  Enqueues only. */
int wmf_row_inv_norms(const float* M, int64_t n, int f, int ld, int bias, float* out, void* stream);

/* Neighbours in factor space: the topn rows of `catalogue` [n_rows, ld] closest to each of n_queries rows of `queries`, by dot
 * product or cosine over the feature columns -- "which items are like this one" (both matrices the item factors) and the same for
 * users.  The reference has no counterpart on the factor model (RecModel offers neighbourhoods through its separate item-KNN
 * model only).  One fused pass: the catalogue scan, the running top-n and the merge of wmf_recommend_topn.
 * Inputs: all arrays on the device, both matrices in the library's layout with the same f and ld; they may be the same matrix.
 *   query_idx[b] selects the row of `queries` that batch position b asks for; a row may occur several times.
 * Dot product: d(b, j) = the sum over the columns c in [bias, f) of queries[query_idx[b], c] * catalogue[j, c], in the score
 *   tile's arithmetic (the operand pattern and MFMA order of wmf_recommend_topn and wmf_predict_pairs).  With bias != 0 column 0 is
 *   left out of the sum and nothing is added: bit for bit wmf_recommend_topn(bias = 0) on copies whose column 0 is zero.
 * Score: q_inv_norm == c_inv_norm == NULL: the score is d (dot product).  Both given (wmf_row_inv_norms of the two matrices):
 *   score = (d * q_inv_norm[query_idx[b]]) * c_inv_norm[j] (cosine) -- two float32 multiplications in exactly that order, after the
 *   sum; q_inv_norm is indexed by the row id, not by the batch position.  One pointer without the other is WMF_EINVAL.
 * Self-exclusion: exclude_self != 0: catalogue row query_idx[b] is never returned for batch position b (meaningful when both
 *   matrices are the same).
 * Exclusion lists: excl_indptr is int64[n_queries + 1]; row b of that CSR belongs to batch position b; excl_indices are catalogue
 *   rows in [0, n_rows), ascending within a row, duplicates allowed; read exactly as wmf_recommend_topn reads its seen list.  Both
 *   pointers or neither (NULL: nothing else is excluded).
 * Order, outputs, limits, slices and workspace are those of wmf_recommend_topn: a higher score wins, equal scores go to the lower
 *   row id (-0.0 and +0.0 are equal); out_rows[b * topn + k] = the k-th best row, out_scores (may be NULL) its score, out_count[b]
 *   (may be NULL) = min(topn, eligible rows), entries past it hold -1 and -inf; 1 <= topn <= WMF_RECOMMEND_MAX_TOPN, n_queries >= 1,
 *   1 <= n_rows < 2^31; n_slices 0 (the library chooses) or 1 .. WMF_RECOMMEND_MAX_SLICES, and the result does not depend on it;
 *   wmf_similar_workspace_bytes(n_queries, topn, n_slices) = wmf_recommend_workspace_bytes of the same arguments.
 * The call only enqueues: it does not allocate, synchronise or read back.  WMF_EINVAL, before any HIP call, for a bad shape, a null
 * pointer, an unpaired pointer, topn or n_slices out of range or a workspace that is too small.
 * Factors and scales are finite; NaN scores are unspecified, but every index written is in range. */
int64_t wmf_similar_workspace_bytes(int64_t n_queries, int64_t topn, int32_t n_slices);
int wmf_similar_topn(const float* queries, const float* catalogue, int f, int ld, int bias,
                     const float* q_inv_norm, const float* c_inv_norm,
                     const int32_t* query_idx, int64_t n_queries, int64_t n_rows,
                     int32_t exclude_self, const int64_t* excl_indptr, const int32_t* excl_indices,
                     int64_t topn, int32_t n_slices,
                     int32_t* out_rows, float* out_scores, int32_t* out_count,
                     void* workspace, int64_t workspace_bytes, void* stream);

/* wmf_similar_topn among the rows an allow mask admits: the mask form of wmf_recommend_topn_filtered over the catalogue's n_rows
 * (allow_bits uint32[n_masks][allow_words], allow_words >= ceil(n_rows / 32), allow_idx int32[n_queries] in [-1, n_masks) or NULL
 * for mask 0 everywhere).  exclude_self still removes the row's own id even when the mask allows it.  allow_bits == NULL (and
 * allow_idx == NULL) is wmf_similar_topn, bit for bit; with a mask the result is, bit for bit, wmf_similar_topn with the masked-out
 * rows appended to every exclusion row.  Everything else -- scores, order, outputs, limits, slices, workspace, refusals -- as
 * wmf_similar_topn; a mask with n_masks < 1 or allow_words too small is WMF_EINVAL before any HIP call.  There is no list form for
 * the scaled score. */
int wmf_similar_topn_filtered(const float* queries, const float* catalogue, int f, int ld, int bias,
                              const float* q_inv_norm, const float* c_inv_norm,
                              const int32_t* query_idx, int64_t n_queries, int64_t n_rows,
                              int32_t exclude_self, const int64_t* excl_indptr, const int32_t* excl_indices,
                              const uint32_t* allow_bits, int64_t allow_words, int32_t n_masks, const int32_t* allow_idx,
                              int64_t topn, int32_t n_slices,
                              int32_t* out_rows, float* out_scores, int32_t* out_count,
                              void* workspace, int64_t workspace_bytes, void* stream);

/* Diversified top-n: greedy Maximal Marginal Relevance (Carbonell & Goldstein 1998) over a candidate pool, the second stage behind
 * wmf_recommend_topn_wide.  A pure top-n of a factor model returns near-duplicates; MMR picks items one by one and trades the
 * relevance of a candidate against its highest similarity to what is already picked.  The reference has no counterpart.  Needs the
 * item factors only: nothing of size rows x pool x f is ever stored.
 * Inputs: all arrays on the device, `items` [n_items, ld] in the library's layout.  Row b owns pool_items[b * pool .. b * pool + pool)
 *   and the pool_scores at the same places: the layout wmf_recommend_topn_wide(topn = pool) writes.
 * Candidates: the candidates of row b are its leading c_b = pool_count[b] entries (values in [0, pool]); pool_count == NULL: all
 *   `pool` entries.  Candidates are numbered by their position j.  Ids lie in [0, n_items); an id listed twice is two candidates.
 *   r_j = pool_scores[b, j] is taken as given: nothing is scored again.
 * Similarity: d(j, s) = the sum over the columns c in [bias, f) of items[id_j, c] * items[id_s, c], in ONE order: of 16 lanes, lane
 *   g takes the 16-byte pieces g, g + 16, ... of the two rows in turn and the four columns of a piece in ascending order, each product
 *   added by one fused multiply-add into the lane's float32 sum (which starts at +0; a column outside [bias, f) enters as a zero
 *   factor); the 16 sums are then added by the butterfly of wmf_predict_pairs, s += s[lane ^ 1], s += s[lane ^ 2], s += s[7 - lane]
 *   within each half of eight lanes, s += s[15 - lane].  With bias != 0 column 0 is the bias and no
 *   feature.  inv_norm == NULL: sim = d (dot product).  inv_norm = wmf_row_inv_norms(items): sim(j, s) = (d * inv_norm[id_j]) *
 *   inv_norm[id_s] (cosine) -- two float32 multiplications in exactly that order, as in wmf_similar_topn; j is the candidate, s the
 *   pick.
 * Greedy selection: mu = 1.0f - lambda in float32.  Step 0: v_j = lambda * r_j.  Step t >= 1: m_j = the largest sim(j, s_i) over the
 *   picks s_0 .. s_{t-1} so far (the first one as it is; a later one replaces m_j only where it compares greater), and v_j = lambda * r_j
 *   - mu * m_j: three separately rounded float32 operations, never a fused multiply-add.  Every step takes the remaining candidate
 *   with the largest v; equal v go to the lower position and -0.0 equals +0.0 (the key of wmf_recommend_topn on v, with the
 *   position in the place of the item id: the library's one total order).  A picked position is never picked again.
 * Outputs: out_count[b] (may be NULL) = min(topn, c_b); out_items[b * topn + k] = the id of pick k; out_scores[b * topn + k] (may be
 *   NULL) = the bits of r of pick k; out_marginal[b * topn + k] (may be NULL) = the v it was picked with; entries past the count hold
 *   -1, -inf, -inf.  lambda = 1 returns the pool's prefix when the pool is sorted (as wmf_recommend_topn_wide leaves it).
 * Limits: 1 <= pool <= WMF_MMR_MAX_POOL, 1 <= topn <= WMF_RECOMMEND_MAX_TOPN, 0 <= lambda <= 1, n_rows >= 1, 1 <= n_items < 2^31.
 * Kernels: one workgroup per row; r_j, m_j, the id with its taken flag and the inverse norm live in LDS (16 bytes a candidate).  pool <=
 *   wmf_rerank_mmr_resident_pool(f, ld) -- pure host code, the rows that fit the 160 KB of a CU beside that state; it does not grow
 *   with ld -- takes the RESIDENT kernel: the candidates' rows are gathered into LDS once and every step reads them there (bytes read
 *   from the table: rows x pool x row).  A larger pool takes the STREAMING kernel, which reads the rows from the table again each
 *   step (rows x pool x (picks - 1) x row).  One body: the two give the same bits; the routing is a function of (f, ld, pool) alone.
 * Determinism: a row's result is a function of that row's inputs alone, not of the batch, the row's position, the grid or timing.
 * The call only enqueues: it does not allocate, synchronise or read back.  WMF_EINVAL, before any HIP call and with the outputs
 * untouched, for a bad shape, a null pointer, lambda outside [0, 1] or NaN, topn or pool out of range.  Factors, scales and scores
 * are finite; non-finite scores or similarities are unspecified, but every index written is in range. */
#define WMF_MMR_MAX_POOL 4096
int64_t wmf_rerank_mmr_resident_pool(int f, int ld);
int wmf_rerank_mmr(const float* items, int64_t n_items, int f, int ld, int bias,
                   const float* inv_norm,
                   const int32_t* pool_items, const float* pool_scores, const int32_t* pool_count,
                   int64_t n_rows, int64_t pool,
                   float lambda, int64_t topn,
                   int32_t* out_items, float* out_scores, float* out_marginal, int32_t* out_count,
                   void* stream);

/* Intra-list similarity, the measure a diversified list is judged by: for row b, over the unordered pairs i < j of the leading n =
 * list_count[b] entries of lists[b * width .. b * width + width) (list_count == NULL: all `width`; values in [0, width]; ids in
 * [0, n_items), an id listed twice is two entries), sim = sim(j, i) of wmf_rerank_mmr -- the same dot, and for the cosine (d *
 * inv_norm[id_j]) * inv_norm[id_i].  out_mean[b] = the mean of sim: S_j = the float64 sum of sim(j, i) over i = 0 .. j - 1 in that
 * order, the total = S_1 + S_2 + ... + S_{n-1} in that order, divided in float64 by n (n - 1) / 2 and rounded to float32 once; 0 for
 * fewer than two entries.  out_max[b] = the largest of those sims (-inf for fewer than two entries).  1 <= width <=
 * WMF_ILS_MAX_WIDTH, n_rows >= 1, 1 <= n_items < 2^31; WMF_EINVAL before any HIP call otherwise, and for a null pointer.  Enqueues
 * only; one workgroup per row. */
#define WMF_ILS_MAX_WIDTH 128
int wmf_intra_list_similarity(const float* items, int64_t n_items, int f, int ld, int bias,
                              const float* inv_norm,
                              const int32_t* lists, const int32_t* list_count,
                              int64_t n_rows, int64_t width,
                              float* out_mean, float* out_max, void* stream);

/* The exact place of held-out items in the full-catalogue order of wmf_recommend_topn: the dual query of that entry point, not
 * "which are the topn best" but "at which place does this item stand", for unsampled, train-excluded Recall / NDCG / ARHR
 * (RecModel.eval_ranking; the reference offers only the sampled Recall@N of base_model.py:100-148).  One counting pass over the
 * catalogue for the whole batch -- scores by f32 MFMA, integer counters; nothing of size n_rows x n_items is ever stored.
 * Inputs: all arrays on the device, factors in the library's layout (ld % 4 == 0, zero padding).  A ROW is a batch position b:
 *   a user (user_idx[b]; a user may occur in several rows), a seen list and a target list.
 * Seen list: as for wmf_recommend_topn -- seen_indptr is int64[n_rows + 1], row b of that CSR belongs to batch position b;
 *   seen_indices are item ids in [0, n_items), ascending within a row, duplicates allowed.  Both NULL: nothing is excluded.
 * Targets: target_indptr is int64[n_rows + 1]; target_indices[target_indptr[b] .. target_indptr[b + 1]) are the item ids of row
 *   b in [0, n_items), in any order, duplicates allowed.  out_rank and out_score are indexed like target_indices.
 * Outputs, for target p of row b:
 *   out_rank[p] = the number of items j of [0, n_items) that are not in row b's seen list and stand strictly above the target in
 *     the order of wmf_recommend_topn (a higher score wins, equal scores go to the lower item id): the 0-based place of the
 *     target in recommend(user, topn = n_items, exclude = seen).  The other targets of the row are ordinary items and are
 *     counted; duplicate targets get the same rank.  For every k <= WMF_RECOMMEND_MAX_TOPN the target is among the first k
 *     entries of wmf_recommend_topn for the same row exactly when 0 <= out_rank[p] < k.
 *     WMF_RANKPOS_SEEN: the target is in the row's seen list and is never recommended.
 *     WMF_RANKPOS_BEYOND: the target lies past the row's first WMF_RANKPOS_MAX_TARGETS targets and was not counted (split
 *     the row; WMF.rank_positions does).
 *   out_score[p] (may be NULL) = the target's score, bit for bit what wmf_recommend_topn and wmf_rank_topn_batch return for the
 *     pair; written for WMF_RANKPOS_SEEN targets too, not for WMF_RANKPOS_BEYOND ones.
 * Limits: n_rows >= 1, 1 <= n_items < 2^31.
 * Slices: as for wmf_recommend_topn (0: the library chooses; 1 .. WMF_RECOMMEND_MAX_SLICES forces it); the counts are
 *   integers, so the result does not depend on n_slices.
 * Workspace: wmf_rank_positions_workspace_bytes(n_rows, n_targets, n_slices) bytes of device memory =
 *   WMF_RANKPOS_WS_BASE + WMF_RANKPOS_WS_PER_ROW * n_rows: it depends neither on n_items nor, with the per-row limit, on the
 *   number of targets or slices.
 * The call only enqueues: it does not allocate, synchronise or read back.  WMF_EINVAL, before any HIP call, for a bad shape, a
 * null pointer (seen_indptr and seen_indices: both or neither), n_slices out of range or a workspace that is too small.
 * Factors are finite; NaN scores are unspecified, but every index read or written is in range. */
#define WMF_RANKPOS_MAX_TARGETS 16
#define WMF_RANKPOS_SEEN (-1)
#define WMF_RANKPOS_BEYOND (-2)
#define WMF_RANKPOS_WS_BASE 256
#define WMF_RANKPOS_WS_PER_ROW 260
int64_t wmf_rank_positions_workspace_bytes(int64_t n_rows, int64_t n_targets, int32_t n_slices);
int wmf_rank_positions(const float* users, const float* items, int f, int ld, int bias,
                       const int32_t* user_idx, int64_t n_rows, int64_t n_items,
                       const int64_t* seen_indptr, const int32_t* seen_indices,
                       const int64_t* target_indptr, const int32_t* target_indices,
                       int32_t n_slices, int32_t* out_rank, float* out_score,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* RecModel.eval_topn / compute_hit, base_model.py:51-148, for all test entries at once.
 * Test entry p = (pair_user[p], pair_item[p]); its user's random candidates are row pair_row[p] of
 * candidates[n_rows][n_cand] (item rows, drawn by the caller exactly as base_model.py:62-63 draws them) and
 * position slot[pair_row[p]] of that row is where the reference writes the test item (:84).
 * hits[t] = number of test entries whose item is among the topn[t] best of its candidate row, i.e. for
 * which fewer than topn[t] of the other n_cand - 1 candidates score strictly higher (:86-93).
 * All arrays on the device; hits is int64[n_topn], n_topn <= 64. */
int wmf_hit_counts(const float* users, const float* items, int f, int ld, int bias,
                   const int32_t* pair_user, const int32_t* pair_item, const int32_t* pair_row, int64_t n_pairs,
                   const int32_t* candidates, int32_t n_cand, const int32_t* slot,
                   const int32_t* topn, int32_t n_topn, int64_t* hits, void* stream);

/* out[i, :] = in[rows[i], :] for i < n: the rows of a freshly solved factor block packed per destination rank, for the
 * need-list exchange of the sharded engine (the parallelism that replaces the reference's Pool, wmf_model.py:245-249): each
 * rank is sent only the rows its own half step reads.  in / out row-major with ld floats per row (ld a multiple of 4),
 * rows int64[n] (indices into `in`; validated by the caller), all on the device.  Enqueues only. */
int wmf_gather_rows(const float* in, int ld, const int64_t* rows, int64_t n, float* out, void* stream);

/* g[u, :] = sum_j values[j] * V[indices[j], :]  (CSR x dense), the SpMM of the un-weighted
 * closed form wmf_model.py:85,88 in whitened coordinates. */
int wmf_spmm_rows(const float* V, const int64_t* indptr, const int32_t* indices, const float* values,
                  int64_t n, int f, int ld, float* g, void* stream);

/* COO -> CSR on the device, stable in (row, column): entry e = (rows[e], cols[e], values[e]), all device arrays.  With
 * (rows, cols) swapped this is the transpose the reference takes before training (wmf_model.py:128, count_mat.T.tocsr());
 * the sharded engine also builds every rank's shards with it.  Duplicates are kept, in their stored order.
 * indptr_out int64[n_rows + 1], indices_out int32[nnz], values_out float[nnz]; n_cols <= 2^31 - 1, n_rows * n_cols < 2^63,
 * nnz < 2^32.  bad_flag (device int32, caller zeroes): set to 1 if an entry lies outside [0, n_rows) x [0, n_cols) -- the
 * outputs are then unspecified (never written out of bounds).  workspace: wmf_coo_to_csr_workspace_bytes() bytes. */
int64_t wmf_coo_to_csr_workspace_bytes(int64_t nnz, int64_t n_rows, int64_t n_cols);
int wmf_coo_to_csr(const int64_t* rows, const int64_t* cols, const float* values, int64_t nnz, int64_t n_rows, int64_t n_cols,
                   int64_t* indptr_out, int32_t* indices_out, float* values_out, int32_t* bad_flag, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* values[i] = alpha*log(1+beta*values[i]) (mode 0) or alpha*values[i] (mode 1), in place on the
 * device.  wmf_model.py:119-123. */
int wmf_confidence_transform(float* values, int64_t nnz, double alpha, double beta, int mode, void* stream);
/* The same on float64 values (the count matrix of a `cores > 1` run stays float64, wmf_model.py:119-123). */
int wmf_confidence_transform_f64(double* values, int64_t nnz, double alpha, double beta, int mode, void* stream);

/* ---- float64 half step: the reference's Pool variants (a5 / a6) ------------------------------------------------------
 * recompute_factors_par / recompute_factors_bias_par (wmf_model.py:242-265) and their row functions
 * recompute_factors_intern / recompute_factors_bias_intern (:267-309): with a float64 count matrix every row is
 *   x_u = solve(Y~^T Y~ + lambda I + Y~_u^T diag(w) Y~_u,  Y~_u^T (w + 1))        in float64,
 * Y~ = Y with column 0 read as 1 and w = c_u - Y[idx, 0] for bias != 0 (:253-257, :279), rows without stored entries
 * are zero (:274-276, :296-298), and the float64 rows are stacked without a cast (np.stack, :246 / :261) -- so the
 * reference's `cores > 1` training continues on float64 factors (cores = 4 is the reference's default, :49-51).  This entry
 * point is that arithmetic on the device, without the whitening of the float32 path: Gramian in float64, then per row
 * the system accumulated and factored in registers, one workgroup or wave per row (blocked Cholesky; rows with at most 32 stored
 * entries through the whitened low-rank form -- a d x d system -- when they are at least a quarter of the rows; a system that is not positive
 * definite -- bias-adjusted weights below zero -- or not finite is redone by LU with partial pivoting, np.linalg.solve's
 * gesv); both agree with the float64 reference arithmetic to 1e-10.
 *   Y [m, f] float64 row-major (dense, no padding), values float64[nnz], X [n, f] float64 out, all on the device;
 *   workspace: wmf_half_step_f64_workspace_bytes(f, m, n) bytes; fail_count (device int32, caller zeroes): += 1 per
 *   exactly singular row system (its X row is NaN; the reference raises LinAlgError).  Enqueues only. */
int64_t wmf_half_step_f64_workspace_bytes(int f, int64_t m, int64_t n);
int wmf_half_step_f64(const double* Y, int64_t m, int f, int bias, const int64_t* indptr, const int32_t* indices,
                      const double* values, int64_t n, double lambda, double* X, void* workspace, int64_t workspace_bytes,
                      int32_t* fail_count, void* stream);
/* The same with host buffers in and out (what recompute_factors_par(Y, C, lambda_reg, cores) is handed, :242):
 * synchronous, allocates and frees its device buffers; WMF_ENUMERIC if a row system was singular. */
int wmf_recompute_factors_f64_host(const double* Y_host, int64_t m, int f, int bias, const int64_t* indptr,
                                   const int32_t* indices, const double* values, int64_t n, double lambda, double* X_host);

/* ---- partial systems for a reduce-scatter exchange (f <= 144) ------------------------------------
 * When the rows being updated are few and the fixed side is large (many users, few items), gathering the fixed
 * side's factors costs more than exchanging the rows' accumulated systems: every rank accumulates, for EVERY row,
 * the part of  V_u^T D V_u  and  V_u^T p  that its own slice of the fixed side contributes, the partial systems are
 * summed over ranks (reduce-scatter), and each rank eliminates the rows it owns.  Same arithmetic as
 * wmf_solve_rows' heavy-row kernel (wmf_model.py:233-239), split at the sum over stored entries.
 *   wmf_partial_row_floats(f)  floats per row of a partial-system buffer (0: width not supported);
 *   wmf_accumulate_rows        slot (i * slot_stride + slot_offset) of `partial` = system of CSR row i over the
 *                              entries given (zeros for an empty row).  slot_stride = 1, slot_offset = 0: one slot per
 *                              row.  Larger strides let several calls -- one per arriving chunk of the fixed side --
 *                              fill different slots of the same rows.  degrees = int32[n] device,
 *                              indptr[i + 1] - indptr[i]; bias_fixed != NULL needs w_eff_workspace (float[nnz], device)
 *                              unless V / bias_fixed are in the split layout of wmf_row_transform;
 *   wmf_eliminate_rows         g[i] = (I + sum of row i's slots_per_row consecutive slots)^-1 (sum of their y), slots
 *                              added in order; a row whose system is not positive definite is counted in fail_count
 *                              (there is no CSR here to hand to the pivoted fallback); scratch = int32[n] device. */
int64_t wmf_partial_row_floats(int f);
int wmf_accumulate_rows(const float* V, const float* bias_fixed, const int64_t* indptr, const int32_t* degrees,
                        const int32_t* indices, const float* values, int64_t n, int64_t nnz, int f, int ld,
                        float* partial, int32_t slot_stride, int32_t slot_offset, float* w_eff_workspace, void* stream);
int wmf_eliminate_rows(float* partial, int64_t n, int32_t slots_per_row, int f, int ld, float* g, int32_t* fail_count,
                       int32_t* scratch, void* stream);

/* ---- per-kernel timing (bench.py roofline) ------------------------------------------------- */
/* While enabled, every kernel launch of the device-level entry points is bracketed by two HIP events on its own
 * stream.  wmf_profile_collect() waits for the events recorded so far, folds them into a table with one entry per
 * (kernel symbol, tag) and returns the number of entries; wmf_profile_entry(i, ...) reads entry i: the kernel's name as
 * rocprofv3 prints it, up to and including its template arguments ("solve_low_kernel<9, 1, false, false>"), the tag,
 * total / min / max milliseconds and the launch count.  The tag is whatever wmf_profile_set_tag() last set (bench.py:
 * 0 = users half step, 1 = items half step), so the launches of one kernel on the two sides are kept apart.
 * wmf_profile_reset() empties the table.  All five are thread-safe. */
int wmf_profile_enable(int on);
int wmf_profile_set_tag(int tag);
int wmf_profile_collect(void);
int wmf_profile_entry(int i, char* name, int name_cap, int* tag, double* ms, int64_t* launches, double* min_ms, double* max_ms);
int wmf_profile_reset(void);
/* Kernel-SELECTION switches (tools/kernel_lab.py, recmodel_amd/_lib.py DEBUG_FLAGS): a bit mask, default 0, process-wide,
 * not synchronised with running solves.  Without the word `lab` a switch is accepted by the shipped library, computes the
 * same results as the default, and is set by a GPU test (tests/test_abi.py checks that each of them occurs in one).  With
 * `lab` it exists only in a -DWMF_LAB build (make -C recmodel_amd/csrc lab): the shipped wmf_debug_set_flags answers
 * WMF_EINVAL for it, and the kernels only it reaches are not compiled in.  (Bit 512 is reserved: it selected the first two
 * generations of the factorisation kernel until they were deleted.) */
enum {
    WMF_DBG_NO_ELIMINATION      = 1,          /* lab  ablation, results WRONG: no elimination */
    WMF_DBG_NO_ACCUMULATION     = 2,          /* lab  ablation, results WRONG: no accumulation MFMAs */
    WMF_DBG_NO_TILE_INVERSE     = 8,          /* lab  ablation, results WRONG: no tile inverse */
    WMF_DBG_LOW32_GAUSS_JORDAN  = 64,         /* lab  plain 32 x 32 Gauss-Jordan for rows with 17 .. 32 entries */
    WMF_DBG_NO_BORDER           = 256,        /* lab  no border column (and so no split layout) at f = 16 m + 1 */
    WMF_DBG_WIDE_EIGHT_WAVES    = 1024,       /* lab  the run-time-indexed eight-wave kernel for every f > 144 */
    WMF_DBG_NO_ROW_PAIRS        = 2048,       /* lab  no two-rows-per-wave kernel for rows with at most 8 entries */
    WMF_DBG_HEAVY_REG_RING      = 4096,       /*      register-ring heavy-row kernel at k = 128 (instead of the LDS-DMA ring) */
    WMF_DBG_HEAVY_F32_ACC       = 8192,       /* lab  f32 MFMA accumulation in the LDS-DMA kernel */
    WMF_DBG_HEAVY_REG_RING_K64  = 65536,      /* lab  register-ring heavy-row kernel at k = 64 (instead of the LDS-DMA ring) */
    WMF_DBG_F32_GRAM            = 131072,     /*      f32 MFMA Gramian for f = 97 .. 144 (instead of split bf16) */
    WMF_DBG_F32_TRANSFORM       = 262144,     /* lab  f32 MFMA row transform for f = 97 .. 144 (no rolled layout then) */
    WMF_DBG_LOW_F32_TILES       = 524288,     /* lab  f32 S tiles for rows with at most 32 entries */
    WMF_DBG_WIDE_F32            = 2097152,    /* lab  f32 MFMA kernel for f > 144 (it does not split rows above 4096 entries) */
    WMF_DBG_HEAVY_ONE_WAVE      = 16777216,   /*      k = 128 heavy-row kernel with 16-entry groups at one wave per SIMD (instead of 8 at two) */
    WMF_DBG_HEAVY_PIVOTED_LU    = 33554432,   /* lab  every row of 33 .. 4096 entries (f <= 144) through the pivoted f32 LU kernel */
    WMF_DBG_F64_TEAMS           = 67108864,   /* lab  float64 half step: workgroup teams at every width */
    WMF_DBG_F64_NO_LOW_RANK     = 134217728,  /*      float64 half step: no whitened low-rank path (nor its iteration), every row by the direct f x f kernels */
    WMF_DBG_NO_ITER             = 268435456,  /*      no matrix-free iteration kernel (csrc/wmf_iter.hip): every row above 32 entries is eliminated */
    WMF_DBG_F64_VALU            = 536870912,  /*      VALU forms of the float64 Gramian and row transform (instead of v_mfma_f64_16x16x4_f64) */
    WMF_DBG_NO_ROLLED_LAYOUT    = 1073741824  /* lab  wmf_rolled_layout_supported() answers 0 (callers keep the plain split layout) */
};
/* Returns WMF_EINVAL, and leaves the switches as they were, for a bit this build does not accept. */
int wmf_debug_set_flags(int flags);
int wmf_debug_get_flags(void);

#ifdef __cplusplus
}
#endif
#endif /* WMF_HIP_H */
