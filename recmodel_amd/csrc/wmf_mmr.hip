// Diversified top-n (gfx950): greedy Maximal Marginal Relevance over a row's candidate pool, and the intra-list similarity of
// finished lists.  Definitions: include/wmf_hip.h, wmf_rerank_mmr and wmf_intra_list_similarity; strides, budget and measurements:
// DESIGN.md section 5.
//
//   * mmr_kernel<NP, RES> -- one 256-thread workgroup per row, grid-stride over the rows.  A row's state lives in LDS: r_j, m_j,
//                            the id of every candidate (the complement of the id once the candidate is picked: the taken
//                            flag) and its inverse norm, 16 bytes a candidate -- the step loop of the resident variant reads
//                            nothing from global memory.  Step 0 picks the largest lambda r_j.  Every later step broadcasts the
//                            row picked last through LDS (`pick`, the columns that are no features zeroed), takes the dot of
//                            every remaining candidate with it -- a 16-lane group per candidate, mmr_dot --, folds it into m_j,
//                            forms v_j and reduces the 64-bit keys (wmf_score_key(v) : ~position) over the workgroup.  Two
//                            barriers a step; min(topn, c_b) - 1 updates.
//       RES = true           the RESIDENT variant: the candidates' rows are gathered into LDS once (raw, ld floats a row) and every
//                            step reads them from there.  Bytes read from the table: rows x pool x row, once.
//       RES = false          the STREAMING variant: the rows are read from the item table again each step (from L2 / Infinity
//                            Cache where the pools of the rows in flight fit them), two candidates and so 2 NP 16-byte loads a
//                            lane in flight.
//                            Bytes read: rows x pool x (picks - 1) x row.
//     One body: the variants differ in where a row's pointer points, so their results are the same bits.
//     A group takes the candidates j0 = 32 i + 16 h + p and j0 + 8 (h = group & 1, p = group >> 1).  The two groups that share
//     one service group of a 16-byte LDS read (ds_read_b128 serves lanes {0-3, 12-15, 20-27} together, {4-11, 16-19, 28-31}
//     together, ...: half of one 16-lane group and half of its neighbour) therefore read rows 16 apart: the same 16-byte slot
//     modulo 256 bytes whatever the row stride, and between them the two halves cover all 64 banks once.  No padding is needed.
//   * ils_kernel<NP>      -- the mean and the largest similarity over the pairs of a list, the same dot; float64 sums per list
//                            position in ascending order of the partner, then over the positions in ascending order.
// No atomics, fixed orders everywhere: a row's result depends on nothing but the row.
#include "wmf_common.h"                     /* wmf_row16_sum */
#include "wmf_internal.h"
#include "wmf_scan.h"                       /* wmf_score_key */

#define WMF_MMR_MAX_BLOCKS 1024             /* workgroups of either kernel: rows beyond it take another trip */
#define MMR_PICK_PIECES 80                  /* 16 lanes x 5 pieces: the broadcast row, zero past the row's ld / 4 pieces */
#define MMR_MAX_NP 5                        /* pieces a lane: ceil(272 / 4 / 16) */
#define MMR_LDS_BUDGET (160 * 1024 - 1024)  /* a CU's LDS less the kernel's static words */

static_assert(MMR_PICK_PIECES == 16 * MMR_MAX_NP && WMF_MMR_MAX_POOL == WMF_RECOMMEND_WIDE_MAX_TOPN, "mmr geometry");

// dynamic LDS of mmr_kernel: pick | r | m | id | inverse norm | (resident: pool rows of ld floats)
static inline size_t mmr_lds_bytes(int64_t pool, int ld, bool resident) {
    const int64_t pool4 = (pool + 3) & ~(int64_t)3;
    return (size_t)(MMR_PICK_PIECES * 16 + 16 * pool4 + (resident ? pool * ld * 4 : 0));
}

// ---- the shared arithmetic ------------------------------------------------------------------------------------------------------
// pieces g, g + 16, ... of a row (global or LDS) into registers; pieces past the row are zero
template <int NP>
__device__ __forceinline__ void mmr_load(float4 (&a)[NP], const float4* row, int nch, int g) {
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int c = g + 16 * k;
        a[k] = c < nch ? row[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
// THE dot of the header: lane g sums its pieces in turn, the four columns of a piece in ascending order, every product by one
// fused multiply-add into a float32 sum that starts at +0; then wmf_row16_sum, the DPP butterfly of wmf_pair_score, over the 16
// lanes (the same bits on every lane: each stage adds the two operands of a pair on both of its lanes).
// `pick` holds zeros in the columns outside [bias, f) and past the row.
template <int NP>
__device__ __forceinline__ float mmr_dot(const float4 (&a)[NP], const float4* pick, int g) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const float4 b = pick[g + 16 * k];
        s = fmaf(a[k].x, b.x, s); s = fmaf(a[k].y, b.y, s); s = fmaf(a[k].z, b.z, s); s = fmaf(a[k].w, b.w, s);
    }
    return wmf_row16_sum(s);
}
// sim(j, s): the dot, or (d * inv_norm[id_j]) * inv_norm[id_s]
__device__ __forceinline__ float mmr_sim(float d, float inv_j, float inv_s, bool cosine) {
    return cosine ? __fmul_rn(__fmul_rn(d, inv_j), inv_s) : d;
}
// v = lambda r - mu m: three roundings, never a fused multiply-add.  Plain operators under the pragma, not __fmul_rn / __fsub_rn:
// those are header functions compiled with contraction allowed, and inlined here their product was fused into the subtraction
// (a v_pk_fma_f32 in the gfx950 code); operations written in this block carry no such licence.
__device__ __forceinline__ float mmr_value(float lambda, float r, float mu, float m) {
#pragma clang fp contract(off)
    const float a = lambda * r;
    const float b = mu * m;
    return a - b;
}
__device__ __forceinline__ unsigned long long mmr_key(float v, int j) {
    return ((unsigned long long)wmf_score_key(v) << 32) | (unsigned long long)(~(uint32_t)j);
}
__device__ __forceinline__ unsigned long long mmr_max64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
// row `src` as the broadcast row: threads 0 .. MMR_PICK_PIECES - 1, the columns that are no features and the pieces past the row zero
__device__ __forceinline__ void mmr_fill_pick(float4* pick, const float4* src, int nch, int f, int bias) {
    const int c = threadIdx.x;
    if (c < MMR_PICK_PIECES) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < nch) {
            v = src[c];
            const int col = 4 * c;
            if (col < bias || col >= f) v.x = 0.f;
            if (col + 1 >= f) v.y = 0.f;
            if (col + 2 >= f) v.z = 0.f;
            if (col + 3 >= f) v.w = 0.f;
        }
        pick[c] = v;
    }
}
__device__ __forceinline__ int mmr_clamp_id(int32_t id, int64_t n_items) { return id < 0 ? 0 : (id >= n_items ? (int)(n_items - 1) : id); }

template <int NP, bool RES>
__global__ __launch_bounds__(256) void mmr_kernel(const float* __restrict__ items, int64_t n_items, int f, int ld, int bias,
                                                  const float* __restrict__ inv_norm, const int32_t* __restrict__ pool_items,
                                                  const float* __restrict__ pool_scores, const int32_t* __restrict__ pool_count, int64_t n_rows,
                                                  int pool, float lambda, int topn, int32_t* __restrict__ out_items, float* __restrict__ out_scores,
                                                  float* __restrict__ out_marginal, int32_t* __restrict__ out_count) {
    extern __shared__ __align__(16) unsigned char mmr_lds[];
    __shared__ unsigned long long s_best[4];
    __shared__ float s_inv;
    const int pool4 = (pool + 3) & ~3, nch = ld >> 2;
    float4* pick = reinterpret_cast<float4*>(mmr_lds);
    float* r = reinterpret_cast<float*>(pick + MMR_PICK_PIECES);
    float* m = r + pool4;
    int32_t* id = reinterpret_cast<int32_t*>(m + pool4);
    float* inv = reinterpret_cast<float*>(id + pool4);
    float4* cand = reinterpret_cast<float4*>(inv + pool4);        // (resident only; 16-byte aligned: pool4 is a multiple of 4)
    const float4* items4 = reinterpret_cast<const float4*>(items);
    const int tid = threadIdx.x, g = tid & 15, grp = tid >> 4, first = 16 * (grp & 1) + (grp >> 1);
    const float mu = __fsub_rn(1.0f, lambda), ninf = -__builtin_inff();
    const bool cosine = inv_norm != nullptr;

    for (int64_t b = blockIdx.x; b < n_rows; b += gridDim.x) {
        int cb = pool_count ? pool_count[b] : pool;
        cb = cb < 0 ? 0 : (cb > pool ? pool : cb);
        const int n_pick = topn < cb ? topn : cb;
        for (int j = tid; j < cb; j += 256) {
            r[j] = pool_scores[b * pool + j];
            const int i = mmr_clamp_id(pool_items[b * pool + j], n_items);
            id[j] = i;
            inv[j] = cosine ? inv_norm[i] : 1.f;
        }
        if (tid == 0 && out_count) out_count[b] = n_pick;
        for (int k = n_pick + tid; k < topn; k += 256) {
            out_items[b * topn + k] = -1;
            if (out_scores) out_scores[b * topn + k] = ninf;
            if (out_marginal) out_marginal[b * topn + k] = ninf;
        }
        __syncthreads();
        if (RES && n_pick > 1) {                                   // the rows into LDS, once; two rows a group in flight
            for (int j0 = first; j0 < cb; j0 += 32) {
                const int j1 = j0 + 8;
                float4 a0[NP], a1[NP];
                mmr_load<NP>(a0, items4 + (int64_t)id[j0] * nch, nch, g);
                if (j1 < cb) mmr_load<NP>(a1, items4 + (int64_t)id[j1] * nch, nch, g);
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const int c = g + 16 * k;
                    if (c < nch) {
                        cand[j0 * nch + c] = a0[k];
                        if (j1 < cb) cand[j1 * nch + c] = a1[k];
                    }
                }
            }
            __syncthreads();
        }

        for (int t = 0; t < n_pick; ++t) {
            unsigned long long best = 0;                           // (every key is above 0: ~position is)
            if (t == 0) {
                for (int j = tid; j < cb; j += 256) best = mmr_max64(best, mmr_key(__fmul_rn(lambda, r[j]), j));
            } else {
                const float inv_s = s_inv;
                for (int j0 = first; j0 < cb; j0 += 32) {
                    const int j1 = j0 + 8;
                    const int i0 = id[j0], i1 = j1 < cb ? id[j1] : -1;   // (negative: picked already, or past the row)
                    float4 a0[NP], a1[NP];
                    float n0 = 1.f, n1 = 1.f;
                    if (i0 >= 0) {
                        mmr_load<NP>(a0, RES ? cand + j0 * nch : items4 + (int64_t)i0 * nch, nch, g);
                        n0 = inv[j0];
                    }
                    if (i1 >= 0) {
                        mmr_load<NP>(a1, RES ? cand + j1 * nch : items4 + (int64_t)i1 * nch, nch, g);
                        n1 = inv[j1];
                    }
                    if (i0 >= 0) {
                        const float sim = mmr_sim(mmr_dot<NP>(a0, pick, g), n0, inv_s, cosine), old = m[j0];
                        const float mj = (t == 1 || sim > old) ? sim : old;
                        if (g == 0) m[j0] = mj;
                        best = mmr_max64(best, mmr_key(mmr_value(lambda, r[j0], mu, mj), j0));
                    }
                    if (i1 >= 0) {
                        const float sim = mmr_sim(mmr_dot<NP>(a1, pick, g), n1, inv_s, cosine), old = m[j1];
                        const float mj = (t == 1 || sim > old) ? sim : old;
                        if (g == 0) m[j1] = mj;
                        best = mmr_max64(best, mmr_key(mmr_value(lambda, r[j1], mu, mj), j1));
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) best = mmr_max64(best, wmf_shfl64(best, (tid & 63) ^ o));
            if ((tid & 63) == 0) s_best[tid >> 6] = best;
            __syncthreads();
            const unsigned long long win = mmr_max64(mmr_max64(s_best[0], s_best[1]), mmr_max64(s_best[2], s_best[3]));
            int p = (int)(~(uint32_t)win);
            p = p < 0 ? 0 : (p >= cb ? cb - 1 : p);               // (a remaining candidate always wins: in range)
            // thread 0 sets the taken flag below while the others read the id: they may see either form of it
            const int raw = id[p], ip = raw < 0 ? ~raw : raw;
            if (tid == 0) {
                out_items[b * topn + t] = ip;
                if (out_scores) out_scores[b * topn + t] = r[p];
                if (out_marginal) out_marginal[b * topn + t] = t == 0 ? __fmul_rn(lambda, r[p]) : mmr_value(lambda, r[p], mu, m[p]);
                id[p] = ~ip;
                s_inv = inv[p];
            }
            if (t + 1 < n_pick) mmr_fill_pick(pick, RES ? cand + p * nch : items4 + (int64_t)ip * nch, nch, f, bias);
            __syncthreads();
        }
        __syncthreads();                                           // the next row of this workgroup rewrites the state
    }
}

// ---- intra-list similarity --------------------------------------------------------------------------------------------------
template <int NP>
__global__ __launch_bounds__(256) void ils_kernel(const float* __restrict__ items, int64_t n_items, int f, int ld, int bias,
                                                  const float* __restrict__ inv_norm, const int32_t* __restrict__ lists,
                                                  const int32_t* __restrict__ list_count, int64_t n_rows, int width, float* __restrict__ out_mean,
                                                  float* __restrict__ out_max) {
    __shared__ __align__(16) float4 pick[MMR_PICK_PIECES];
    __shared__ double s_sum[WMF_ILS_MAX_WIDTH];
    __shared__ float s_max[WMF_ILS_MAX_WIDTH];
    __shared__ int s_id[WMF_ILS_MAX_WIDTH];
    __shared__ float s_inv[WMF_ILS_MAX_WIDTH];
    const float4* items4 = reinterpret_cast<const float4*>(items);
    const int nch = ld >> 2, tid = threadIdx.x, g = tid & 15, grp = tid >> 4, first = 16 * (grp & 1) + (grp >> 1);
    const bool cosine = inv_norm != nullptr;
    const float ninf = -__builtin_inff();

    for (int64_t b = blockIdx.x; b < n_rows; b += gridDim.x) {
        int n = list_count ? list_count[b] : width;
        n = n < 0 ? 0 : (n > width ? width : n);
        if (tid < n) {
            const int i = mmr_clamp_id(lists[b * width + tid], n_items);
            s_id[tid] = i;
            s_inv[tid] = cosine ? inv_norm[i] : 1.f;
            s_sum[tid] = 0.0;
            s_max[tid] = ninf;
        }
        __syncthreads();
        for (int i = 0; i + 1 < n; ++i) {                          // entry i against every later entry j: sim(j, i)
            const int ii = s_id[i];
            mmr_fill_pick(pick, items4 + (int64_t)ii * nch, nch, f, bias);
            const float inv_i = s_inv[i];
            __syncthreads();
            for (int j0 = i + 1 + first; j0 < n; j0 += 32) {
                const int j1 = j0 + 8;
                const int i0 = s_id[j0], i1 = j1 < n ? s_id[j1] : -1;
                float4 a0[NP], a1[NP];
                float n0 = 1.f, n1 = 1.f;
                mmr_load<NP>(a0, items4 + (int64_t)i0 * nch, nch, g);
                n0 = s_inv[j0];
                if (i1 >= 0) {
                    mmr_load<NP>(a1, items4 + (int64_t)i1 * nch, nch, g);
                    n1 = s_inv[j1];
                }
                const float sim0 = mmr_sim(mmr_dot<NP>(a0, pick, g), n0, inv_i, cosine);
                if (g == 0) {
                    s_sum[j0] += (double)sim0;
                    if (sim0 > s_max[j0]) s_max[j0] = sim0;
                }
                if (i1 >= 0) {
                    const float sim1 = mmr_sim(mmr_dot<NP>(a1, pick, g), n1, inv_i, cosine);
                    if (g == 0) {
                        s_sum[j1] += (double)sim1;
                        if (sim1 > s_max[j1]) s_max[j1] = sim1;
                    }
                }
            }
            __syncthreads();                                       // the next entry rewrites the broadcast row
        }
        if (tid == 0) {
            double total = 0.0;
            float mx = ninf;
            for (int j = 1; j < n; ++j) {
                total += s_sum[j];
                if (s_max[j] > mx) mx = s_max[j];
            }
            out_mean[b] = n < 2 ? 0.f : (float)(total / (double)((int64_t)n * (n - 1) / 2));
            out_max[b] = mx;
        }
        __syncthreads();
    }
}

// ---- routing and launchers ----------------------------------------------------------------------------------------------------
// the largest pool whose rows, with the per-candidate state, fit the budget: a pure function of ld (0: a shape no kernel takes)
int64_t wmf_mmr_resident_pool(int f, int ld) {
    if (f < 1 || f > WMF_MAX_F || ld < f || (ld & 3) || ld > 272) return 0;
    int64_t p = (MMR_LDS_BUDGET - MMR_PICK_PIECES * 16) / (4 * (int64_t)ld + 16);
    while (p > 0 && mmr_lds_bytes(p, ld, true) > (size_t)MMR_LDS_BUDGET) --p;
    return p < WMF_MMR_MAX_POOL ? p : WMF_MMR_MAX_POOL;
}

int wmf_launch_mmr(const float* items, int64_t n_items, int f, int ld, int bias, const float* inv_norm, const int32_t* pool_items,
                   const float* pool_scores, const int32_t* pool_count, int64_t n_rows, int64_t pool, float lambda, int64_t topn,
                   int32_t* out_items, float* out_scores, float* out_marginal, int32_t* out_count, hipStream_t st) {
    const int64_t grid = n_rows < WMF_MMR_MAX_BLOCKS ? n_rows : WMF_MMR_MAX_BLOCKS;
    const bool resident = pool <= wmf_mmr_resident_pool(f, ld);
    const size_t lds = mmr_lds_bytes(pool, ld, resident);
    return wmf_dispatch_nfb<1, MMR_MAX_NP>((ld / 4 + 15) / 16, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        if (resident) {
            static const char* name = wmf_kname("mmr_kernel<%d, true>", NP);
            WMF_LAUNCH_LDS(name, (mmr_kernel<NP, true>), MMR_LDS_BUDGET, dim3((unsigned)grid), dim3(256), lds, st, items, n_items, f, ld,
                           bias ? 1 : 0, inv_norm, pool_items, pool_scores, pool_count, n_rows, (int)pool, lambda, (int)topn, out_items,
                           out_scores, out_marginal, out_count);
        } else {
            static const char* name = wmf_kname("mmr_kernel<%d, false>", NP);
            WMF_LAUNCH_LDS(name, (mmr_kernel<NP, false>), MMR_LDS_BUDGET, dim3((unsigned)grid), dim3(256), lds, st, items, n_items, f, ld,
                           bias ? 1 : 0, inv_norm, pool_items, pool_scores, pool_count, n_rows, (int)pool, lambda, (int)topn, out_items,
                           out_scores, out_marginal, out_count);
        }
        return (int)WMF_L_OK;
    });
}

int wmf_launch_ils(const float* items, int64_t n_items, int f, int ld, int bias, const float* inv_norm, const int32_t* lists,
                   const int32_t* list_count, int64_t n_rows, int64_t width, float* out_mean, float* out_max, hipStream_t st) {
    const int64_t grid = n_rows < WMF_MMR_MAX_BLOCKS ? n_rows : WMF_MMR_MAX_BLOCKS;
    (void)f;
    return wmf_dispatch_nfb<1, MMR_MAX_NP>((ld / 4 + 15) / 16, [&](auto np) {
        constexpr int NP = decltype(np)::value;
        static const char* name = wmf_kname("ils_kernel<%d>", NP);
        WMF_LAUNCH(name, (ils_kernel<NP>), dim3((unsigned)grid), dim3(256), 0, st, items, n_items, f, ld, bias ? 1 : 0, inv_norm, lists,
                   list_count, n_rows, (int)width, out_mean, out_max);
        return (int)WMF_L_OK;
    });
}
