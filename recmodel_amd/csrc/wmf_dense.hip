// Dense shared-work kernels of one ALS half step (gfx950):
//   gram       G_sum = Y~^T Y~                      f32 MFMA, fp64 cross-wave reduction
//   factorize  G_sum + lambda I = L L^T (fp64), W_white = L^-T, W_unwhite = L^-1 (fp32 out)
//   transform  out = in~ . W                        f32 MFMA, W staged in LDS
// Reference arithmetic: RecModel/wmf_model.py:215 and :328-332 (Gramian of the fixed side, bias
// column forced to one), and the shared part of the per-row solve (:239, :350).
#include "wmf_common.h"
#include "wmf_internal.h"

#include <type_traits>
#include <utility>

// ------------------------------------------------------------------------------------------ gram
// One wave per workgroup.  A wave walks a contiguous range of 4-row steps; at each step lane
// (r = l & 15, q = l >> 4) loads Y~[4s + q][16 fb + r] for every 16-column feature block fb.  The
// same registers are both MFMA operands: tile(bi, bj) += frag[bi]^T frag[bj].  Tiles with
// bi <= bj only.  Each wave writes its partial tiles to `partial`; gram_reduce sums them in fp64.
template <int NFB, int NSPLIT, int S>
__device__ __forceinline__ void gram_body(const float* __restrict__ Y, int64_t m, int f, int ld, int bias,
                                          float* __restrict__ partial, int64_t step_lo, int64_t step_hi) {
    constexpr int NT = NFB * (NFB + 1) / 2;
    constexpr int NACC = (NT + NSPLIT - 1) / NSPLIT;
    const int lane = threadIdx.x & 63;                           // (NSPLIT = 4: the four waves of a workgroup, one tile quarter each)
    const int r = lane & 15, q = lane >> 4;
    f32x4 acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // U steps (4 rows each) per trip; the loads of the next trip are issued before this trip's MFMAs and
    // stay untouched until then (raw loads: masks and the bias column are applied at use).
    constexpr int U = 4;
    float cur[U][NFB], nxt[U][NFB];
    const int last_col = min(16 * (NFB - 1) + r, ld - 1);
    const float col_mask_last = (16 * (NFB - 1) + r < f) ? 1.f : 0.f;
    auto load_trip = [&](int64_t s0, float (&fr)[U][NFB]) {
#pragma unroll
        for (int uu = 0; uu < U; ++uu) {
            const int64_t row = min(4 * (s0 + uu) + q, m - 1);                        // clamped: masked at use
            const float* yrow = Y + row * (int64_t)ld;
#pragma unroll
            for (int fb = 0; fb < NFB - 1; ++fb) fr[uu][fb] = yrow[16 * fb + r];
            fr[uu][NFB - 1] = yrow[last_col];
        }
    };
    if (step_lo < step_hi) load_trip(step_lo, cur);
    for (int64_t s0 = step_lo; s0 < step_hi; s0 += U) {
        if (s0 + U < step_hi) load_trip(s0 + U, nxt);
#pragma unroll
        for (int uu = 0; uu < U; ++uu) {
            const int64_t s = s0 + uu;
            const float rmask = (s < step_hi && 4 * s + q < m) ? 1.f : 0.f;
            float frag[NFB];
#pragma unroll
            for (int fb = 0; fb < NFB; ++fb) frag[fb] = cur[uu][fb] * rmask;
            frag[NFB - 1] *= col_mask_last;
            if (bias && r == 0) frag[0] = rmask;                                     // column 0 reads as 1 (wmf_model.py:331)
            int t = 0;
#pragma unroll
            for (int bi = 0; bi < NFB; ++bi) {
#pragma unroll
                for (int bj = bi; bj < NFB; ++bj, ++t) {
                    if (t % NSPLIT == S) acc[t / NSPLIT] = WMF_MFMA16(frag[bi], frag[bj], acc[t / NSPLIT]);
                }
            }
        }
#pragma unroll
        for (int uu = 0; uu < U; ++uu)
#pragma unroll
            for (int fb = 0; fb < NFB; ++fb) cur[uu][fb] = nxt[uu][fb];
    }
    // partial layout: [wave][tile][reg][lane]
    float* out = partial + (int64_t)blockIdx.x * NT * 256;
    int t = 0;
#pragma unroll
    for (int bi = 0; bi < NFB; ++bi) {
#pragma unroll
        for (int bj = bi; bj < NFB; ++bj, ++t) {
            if (t % NSPLIT == S) {
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) out[(t * 4 + reg) * 64 + lane] = acc[t / NSPLIT][reg];
            }
        }
    }
}

// The same Gramian with split-bf16 products (wide factors, where the f32 MFMAs of gram_body are what bounds the kernel:
// 1.6 ms for 11 M rows at f = 129): a chunk of 32 rows per trip, lane (r, q) loads Y~[32 c + 8 q + j][16 fb + r], j = 0..7
// -- the K index of a 16x16x32 MFMA -- splits every value into three bf16 parts (exact) and issues six bf16 MFMAs per tile
// (lo.hi, mid.mid, hi.lo, mid.hi, hi.mid, hi.hi; the dropped products are below 2^-24 of the term): the accuracy of the
// f32 path at 6 x 16 instead of 8 x 32 MFMA cycles per tile and 32 rows.
typedef __bf16 gram_bf16x8 __attribute__((ext_vector_type(8)));
// The next chunk of a wave is requested while this one is worked on, in two groups: its first feature blocks ahead of this
// chunk's split, the others ahead of its MFMAs.  A chunk is 8 NFB (72) loads and vmcnt counts 63: requested together ahead of
// the split, the split's waits for THIS chunk could only be written as counts that also retire most of the next one, and the
// MFMAs ran with nothing in flight.  Loads return in order and nothing before the last MFMA of a trip reads the next chunk, so
// no wait of a trip asks for one of its loads; they are collected after the MFMAs, when `nxt` becomes `cur` (scheduling fences
// keep the four phases apart: hipcc would otherwise hoist the copies, and their waits, into the split).  The wave's last chunk
// is peeled: the loads inside the loop are unconditional (a conditional request makes the waits of the split cover the path
// without it: all landed), and a chunk that has a successor in its wave is full (c0 + 32 <= c0 + stride < m) -- it is split as
// loaded, its bias column is the constant one; only the peeled chunk, among them the one ragged chunk of the matrix, carries
// the row masks (x * 1.0f is x: the results are the same bits).
// (Two named register sets with the loop unrolled by two, which would drop the copies, spill: the VALU addresses 256 of the 512
// registers, and two raw chunks + the parts + their addresses need 270 of them; measured figures in DESIGN.md section 9.)
// AUG (the Gramian of a solved side's g, wmf_gram_whitened): `f` counts the augmented columns, position f - 1 reads as 1 when
// `bias` is set (column 0 is read as stored), and columns past f are replaced, not multiplied away: g's padding is not trusted.
template <int NFB, bool AUG = false>
__device__ __forceinline__ void gram_body6(const float* __restrict__ Y, int64_t m, int f, int ld, int bias,
                                           float* __restrict__ partial, int64_t step_lo, int64_t step_hi) {
    constexpr int NT = NFB * (NFB + 1) / 2;
    constexpr int NG1 = (5 * NFB + 4) / 9;                                      // feature blocks of the first group: 5 of 9, 4 of 8 and 7
    const int lane = threadIdx.x;
    const int r = lane & 15, q = lane >> 4;
    f32x4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int last_col = min(16 * (NFB - 1) + r, ld - 1);
    const float col_mask_last = (16 * (NFB - 1) + r < f) ? 1.f : 0.f;
    const bool bias_lane = bias && r == (AUG ? (f - 1) & 15 : 0);
    constexpr int ONE_FB = AUG ? NFB - 1 : 0;                                   // the feature block of the column that reads as 1
    // chunks of 32 rows dealt round-robin over the waves (step_lo = this wave, step_hi = the number of waves): at any moment the
    // resident waves read one contiguous stretch of the matrix
    const int64_t stride = 32 * step_hi;
    auto load_blocks = [&](int64_t c0, float (&fr)[8][NFB], int fb_lo, int fb_hi) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t row = min(c0 + 8 * q + j, m - 1);                     // clamped: masked at use
            const float* yrow = Y + row * (int64_t)ld;
#pragma unroll
            for (int fb = 0; fb < NFB; ++fb)
                if (fb >= fb_lo && fb < fb_hi) fr[j][fb] = yrow[fb == NFB - 1 ? last_col : 16 * fb + r];
        }
    };
    auto split = [&](int64_t c0, const float (&fr)[8][NFB], auto masked, gram_bf16x8 (&hi)[NFB], gram_bf16x8 (&mid)[NFB],
                     gram_bf16x8 (&lo)[NFB]) {
        // block by block, as the two load groups arrive; the eight raw values of a block die as its twelve part registers fill
#pragma unroll
        for (int fb = 0; fb < NFB; ++fb) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float rmask = (!decltype(masked)::value || c0 + 8 * q + j < m) ? 1.f : 0.f;
                float x = fr[j][fb];
                if (decltype(masked)::value) x *= rmask;
                if (fb == NFB - 1) x = AUG ? (col_mask_last != 0.f ? x : 0.f) : x * col_mask_last;
                if (fb == ONE_FB && bias_lane) x = rmask;                       // column 0 reads as 1 (wmf_model.py:331)
                const __bf16 h = (__bf16)x;
                const float r1 = x - (float)h;
                const __bf16 md = (__bf16)r1;
                hi[fb][j] = h; mid[fb][j] = md; lo[fb][j] = (__bf16)(r1 - (float)md);
            }
        }
    };
    auto products = [&](const gram_bf16x8 (&hi)[NFB], const gram_bf16x8 (&mid)[NFB], const gram_bf16x8 (&lo)[NFB]) {
        // product-major within a block row: consecutive MFMAs write different accumulators (six in a row on one tile wait
        // for each other's result)
        int t0 = 0;
#pragma unroll
        for (int bi = 0; bi < NFB; ++bi) {
#pragma unroll
            for (int bj = bi; bj < NFB; ++bj) acc[t0 + bj - bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo[bi], hi[bj], acc[t0 + bj - bi], 0, 0, 0);
#pragma unroll
            for (int bj = bi; bj < NFB; ++bj) acc[t0 + bj - bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mid[bi], mid[bj], acc[t0 + bj - bi], 0, 0, 0);
#pragma unroll
            for (int bj = bi; bj < NFB; ++bj) acc[t0 + bj - bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi[bi], lo[bj], acc[t0 + bj - bi], 0, 0, 0);
#pragma unroll
            for (int bj = bi; bj < NFB; ++bj) acc[t0 + bj - bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(mid[bi], hi[bj], acc[t0 + bj - bi], 0, 0, 0);
#pragma unroll
            for (int bj = bi; bj < NFB; ++bj) acc[t0 + bj - bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi[bi], mid[bj], acc[t0 + bj - bi], 0, 0, 0);
#pragma unroll
            for (int bj = bi; bj < NFB; ++bj) acc[t0 + bj - bi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi[bi], hi[bj], acc[t0 + bj - bi], 0, 0, 0);
            t0 += NFB - bi;
        }
    };
    float cur[8][NFB], nxt[8][NFB];
    int64_t c0 = 32 * step_lo;
    if (c0 < m) {
        load_blocks(c0, cur, 0, NFB);
        for (; c0 + stride < m; c0 += stride) {
            gram_bf16x8 hi[NFB], mid[NFB], lo[NFB];
            load_blocks(c0 + stride, nxt, 0, NG1);
            __builtin_amdgcn_sched_barrier(0);
            split(c0, cur, std::false_type{}, hi, mid, lo);
            __builtin_amdgcn_sched_barrier(0);
            load_blocks(c0 + stride, nxt, NG1, NFB);
            __builtin_amdgcn_sched_barrier(0);
            products(hi, mid, lo);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int fb = 0; fb < NFB; ++fb) cur[j][fb] = nxt[j][fb];
        }
        gram_bf16x8 hi[NFB], mid[NFB], lo[NFB];
        split(c0, cur, std::true_type{}, hi, mid, lo);
        products(hi, mid, lo);
    }
    float* out = partial + (int64_t)blockIdx.x * NT * 256;                     // partial layout: [wave][tile][reg][lane]
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) out[(t * 4 + reg) * 64 + lane] = acc[t][reg];
}

template <int NFB>
__global__ __launch_bounds__(64) void gram6_kernel(const float* __restrict__ Y, int64_t m, int f, int ld, int bias,
                                                   float* __restrict__ partial, int64_t steps_per_wave) {
    gram_body6<NFB>(Y, m, f, ld, bias, partial, blockIdx.x, gridDim.x);
}

template <int NFB>
__global__ __launch_bounds__(64) void gram6_aug_kernel(const float* __restrict__ g, int64_t m, int f1, int ld, int bias,
                                                       float* __restrict__ partial) {
    gram_body6<NFB, true>(g, m, f1, ld, bias, partial, blockIdx.x, gridDim.x);
}

// NSPLIT = 4 (f > 144: 136 tiles do not fit one wave's registers): the tile quarters are the FOUR WAVES OF ONE WORKGROUP, which
// walk the same rows at the same time -- one of them brings a row in from HBM, the other three find it in the CU's L1 / L2
// (round 2 launched the quarters as four separate workgroups: 8.26 GB of counted traffic for a 2.05 GB matrix at cfg5s).
template <int NFB, int NSPLIT>
__global__ __launch_bounds__(NSPLIT == 1 ? 64 : 256) void gram_kernel(const float* __restrict__ Y, int64_t m, int f, int ld, int bias,
                                                  float* __restrict__ partial, int64_t steps_per_wave) {
    const int64_t nsteps = (m + 3) / 4;
    int64_t lo = (int64_t)blockIdx.x * steps_per_wave;
    int64_t hi = lo + steps_per_wave;
    if (hi > nsteps) hi = nsteps;
    if (lo > hi) lo = hi;
    if constexpr (NSPLIT == 1) {
        gram_body<NFB, 1, 0>(Y, m, f, ld, bias, partial, lo, hi);
    } else {
        switch (__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) {
            case 0: gram_body<NFB, NSPLIT, 0>(Y, m, f, ld, bias, partial, lo, hi); break;
            case 1: gram_body<NFB, NSPLIT, 1>(Y, m, f, ld, bias, partial, lo, hi); break;
            case 2: gram_body<NFB, NSPLIT, 2>(Y, m, f, ld, bias, partial, lo, hi); break;
            default: gram_body<NFB, NSPLIT, 3>(Y, m, f, ld, bias, partial, lo, hi); break;
        }
    }
}

// G_sum[i][j] (fp64) = sum over waves of the partial tile element; symmetric fill.  Two stages so
// that the sum over up to 1024 waves is spread over the chip: stage 1 sums a slice of the waves
// per (element, slice), stage 2 adds the slices in a fixed order (reproducible).
#define WMF_GRAM_SLICES 32
__global__ __launch_bounds__(256) void gram_reduce1_kernel(const float* __restrict__ partial, int nwaves, int f, int nfb,
                                                           double* __restrict__ slices) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= f * f) return;
    int i = e / f, j = e % f;
    if (i > j) { int tmp = i; i = j; j = tmp; }
    const int bi = i >> 4, bj = j >> 4, ri = i & 15, cj = j & 15;
    // index of tile (bi, bj), bi <= bj, in row-major enumeration of the upper triangle
    const int t = bi * nfb - (bi * (bi - 1)) / 2 + (bj - bi);
    const int lane = cj + 16 * (ri >> 2), reg = ri & 3;
    const int nt = nfb * (nfb + 1) / 2;
    const float* p = partial + ((int64_t)t * 4 + reg) * 64 + lane;
    const int per = (nwaves + WMF_GRAM_SLICES - 1) / WMF_GRAM_SLICES;
    const int w0 = blockIdx.y * per, w1 = min(nwaves, w0 + per);
    double s = 0.0;
    for (int w = w0; w < w1; ++w) s += (double)p[(int64_t)w * nt * 256];
    slices[(int64_t)blockIdx.y * f * f + e] = s;
}

__global__ __launch_bounds__(256) void gram_reduce2_kernel(const double* __restrict__ slices, int f, double* __restrict__ G) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= f * f) return;
    double s = 0.0;
#pragma unroll 8
    for (int k = 0; k < WMF_GRAM_SLICES; ++k) s += slices[(int64_t)k * f * f + e];
    G[e] = s;
}

template <int NFB>
static int launch_gram_nfb(const float* Y, int64_t m, int f, int ld, int bias, float* partial, int nwaves,
                           hipStream_t st) {
    const int64_t nsteps = (m + 3) / 4;
    const int64_t spw = (nsteps + nwaves - 1) / nwaves;
    if constexpr (NFB >= 7 && NFB <= 9) {                     // wide and still one accumulator set per wave: split-bf16 products
        if (!(wmf_debug_flags & WMF_DBG_F32_GRAM)) {          // (WMF_DBG_F32_GRAM, 131072: the f32 MFMA kernel)
            static const char* nm = wmf_kname("gram6_kernel<%d>", NFB);
            WMF_LAUNCH(nm, (gram6_kernel<NFB>), dim3(nwaves), dim3(64), 0, st, Y, m, f, ld, bias, partial, spw);
            return WMF_L_OK;
        }
    }
    if constexpr (NFB <= 9) {
        static const char* nm = wmf_kname("gram_kernel<%d, 1>", NFB);
        WMF_LAUNCH(nm, (gram_kernel<NFB, 1>), dim3(nwaves), dim3(64), 0, st, Y, m, f, ld, bias, partial, spw);
    } else {
        static const char* nm = wmf_kname("gram_kernel<%d, 4>", NFB);
        WMF_LAUNCH(nm, (gram_kernel<NFB, 4>), dim3(nwaves), dim3(256), 0, st, Y, m, f, ld, bias, partial, spw);
    }
    return WMF_L_OK;
}

int wmf_gram_max_waves(int f) {            // keep the per-wave partial tiles within 64 MiB
    const int64_t nfb = (f + 15) / 16, nt = nfb * (nfb + 1) / 2;
    int64_t cap = ((int64_t)64 << 20) / (nt * 1024);
    if (cap > WMF_GRAM_MAX_WAVES) cap = WMF_GRAM_MAX_WAVES;
    return (int)(cap < 64 ? 64 : cap);
}

int wmf_gram_nwaves(int64_t m, int f) {
    int64_t nsteps = (m + 3) / 4;
    int64_t want = (nsteps + 31) / 32;     // at least 32 steps (128 rows) per wave
    if (want < 1) want = 1;
    const int cap = wmf_gram_max_waves(f);
    if (want > cap) want = cap;
    // every wave gets the same share of the rows up front, so the count is a whole number of waves per SIMD (256 CUs x 4):
    // 1456 waves of the wide kernel (one resident wave per SIMD) ran as two rounds, the second 42 % full
    if (want > 1024) want -= want % 1024;
    return (int)want;
}

int wmf_launch_gram(const float* Y, int64_t m, int f, int ld, int bias, double* G_sum, float* partial, double* slices,
                    hipStream_t st) {
    if (m <= 0) return hipMemsetAsync(G_sum, 0, (size_t)f * f * sizeof(double), st) == hipSuccess ? WMF_L_OK : WMF_L_NO_KERNEL;   // (reported as "unsupported f", as ever)
    const int nfb = (f + 15) / 16;
    const int nwaves = wmf_gram_nwaves(m, f);
    if (const int rc = wmf_dispatch_nfb<1, 17>(nfb, [&](auto n) { return launch_gram_nfb<decltype(n)::value>(Y, m, f, ld, bias, partial, nwaves, st); })) return rc;
    WMF_LAUNCH("gram_reduce1_kernel", gram_reduce1_kernel, dim3((f * f + 255) / 256, WMF_GRAM_SLICES), dim3(256), 0, st, partial,
               nwaves, f, nfb, slices);
    WMF_LAUNCH("gram_reduce2_kernel", gram_reduce2_kernel, dim3((f * f + 255) / 256), dim3(256), 0, st, slices, f, G_sum);
    return WMF_L_OK;
}

// G_aug = a^T a over the rows of a solved side, a = [g, 1] (bias) or g: (f + bias)^2 doubles.  The workspace is laid out for
// f + 1 columns (wmf_api.hip).
int wmf_launch_gram_aug(const float* g, int64_t m, int f, int ld, int bias, double* G_aug, float* partial, double* slices,
                        hipStream_t st) {
    const int f1 = f + (bias ? 1 : 0), nfb = (f1 + 15) / 16;
    if (nfb < 7 || nfb > 9) return WMF_L_NO_KERNEL;
    if (m <= 0) return hipMemsetAsync(G_aug, 0, (size_t)f1 * f1 * sizeof(double), st) == hipSuccess ? WMF_L_OK : WMF_L_NO_KERNEL;
    const int nwaves = wmf_gram_nwaves(m, f1);
    if (const int rc = wmf_dispatch_nfb<7, 9>(nfb, [&](auto n) {
            constexpr int NFB = decltype(n)::value;
            static const char* nm = wmf_kname("gram6_aug_kernel<%d>", NFB);
            WMF_LAUNCH(nm, (gram6_aug_kernel<NFB>), dim3(nwaves), dim3(64), 0, st, g, m, f1, ld, bias, partial);
            return (int)WMF_L_OK;
        })) return rc;
    WMF_LAUNCH("gram_reduce1_kernel", gram_reduce1_kernel, dim3((f1 * f1 + 255) / 256, WMF_GRAM_SLICES), dim3(256), 0, st, partial,
               nwaves, f1, nfb, slices);
    WMF_LAUNCH("gram_reduce2_kernel", gram_reduce2_kernel, dim3((f1 * f1 + 255) / 256), dim3(256), 0, st, slices, f1, G_aug);
    return WMF_L_OK;
}

// ------------------------------------------------------------------------------------- factorize
// a double of another lane: v_readlane on its two halves
__device__ __forceinline__ double rl_f64(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// ---- f <= 64, blocked: 16 x 16 blocks, fp64 MFMA for every block product -------------------------------
// A register-resident version of the whole 64 x 64 problem (one lane per row, every (column, row) pair of both sweeps
// unrolled; deleted, see git log) was 32 000 instructions long: four times the instruction cache, so it ran at fetch
// speed (0.12 ms).  Here only the 16 x 16 diagonal blocks are factored and inverted with unrolled scalar code (one copy,
// called per block); panels, trailing updates and the block forward substitution of L^-1 are v_mfma_f64_16x16x4_f64 products
// on tiles in LDS.
//   A operand: lane (r = l & 15, q = l >> 4) supplies A[r][4 kk + q];  B: B[4 kk + q][r];
//   D: lane holds D[q + 4 v][r] in element v (the f64 form's row order differs from the f32 one).
typedef double f64x4 __attribute__((ext_vector_type(4)));
#define WMF_MFMA16_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)
constexpr int FZ_LD = 66;                              // row stride (doubles) of the 64 x 64 LDS images

// Tiles are 16 x 16 windows of row-major images with row strides la / lb / lt (doubles).
// D (+)= A . B^T : D[m][n] = sum_k A[m][k] B[n][k]
__device__ __forceinline__ f64x4 fz_mul_abt(const double* A, int la, const double* B, int lb, f64x4 c, int r, int q, double sign) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) c = WMF_MFMA16_F64(sign * A[r * la + 4 * kk + q], B[r * lb + 4 * kk + q], c);
    return c;
}
// D (+)= A . B : D[m][n] = sum_k A[m][k] B[k][n]
__device__ __forceinline__ f64x4 fz_mul_ab(const double* A, int la, const double* B, int lb, f64x4 c, int r, int q, double sign) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) c = WMF_MFMA16_F64(sign * A[r * la + 4 * kk + q], B[(4 * kk + q) * lb + r], c);
    return c;
}
__device__ __forceinline__ f64x4 fz_load(const double* T, int lt, int r, int q) {
    return f64x4{T[q * lt + r], T[(q + 4) * lt + r], T[(q + 8) * lt + r], T[(q + 12) * lt + r]};
}
__device__ __forceinline__ void fz_store(double* T, int lt, const f64x4& c, int r, int q) {
#pragma unroll
    for (int v = 0; v < 4; ++v) T[(q + 4 * v) * lt + r] = c[v];
}
// Cholesky of the 16 x 16 block D (lower part read) -> L into Lt (upper part zeroed), L^-1 into Xt.  Lane i < 16
// owns row i of D and L; lane j builds column j of the inverse.  One copy of the unrolled code for all blocks.
// Returns 0, or K + 1 for the first column K of the block whose pivot is not positive (wave-uniform).
__device__ __noinline__ int fz_diag(const double* D, double* Lt, double* Xt, int lt, int lane) {
    const int row = lane & 15;
    double a[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) a[j] = D[row * lt + j];
    int fail = 0;
    double rinv[16];                                               // 1 / L[K][K]: the substitution below multiplies by it
#pragma unroll
    for (int K = 0; K < 16; ++K) {
        const double dk = rl_f64(a[K], K);
        if (!(dk > 0.0) && !fail) fail = K + 1;
        // 1 / sqrt(dk): hardware estimate + two Newton steps (full double precision; the library sqrt and divide are
        // each a long dependent sequence, and this chain is serial over the 16 columns)
        double y = __builtin_amdgcn_rsq(dk);
        y = y * (1.5 - 0.5 * dk * y * y);
        y = y * (1.5 - 0.5 * dk * y * y);
        rinv[K] = y;
        a[K] *= y;                                                  // lane K: sqrt(dk); lanes > K: L[i][K]
#pragma unroll
        for (int j = K + 1; j < 16; ++j) a[j] -= a[K] * rl_f64(a[K], j);
    }
    double x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        double sacc = (i == row) ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < i; ++k) sacc -= rl_f64(a[k], i) * x[k];
        x[i] = sacc * rinv[i];
    }
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            Lt[row * lt + j] = (j <= row) ? a[j] : 0.0;           // row `row` of L
            Xt[j * lt + row] = x[j];                               // column `row` of L^-1 (zero above the diagonal)
        }
    }
    return fail;
}

__global__ __launch_bounds__(64, 1) void factorize64m_kernel(const double* __restrict__ G, int f, int ld, double lambda,
                                                             float* __restrict__ Wwhite, float* __restrict__ Wunwhite,
                                                             int32_t* __restrict__ info) {
    __shared__ __attribute__((aligned(16))) double Gs[64 * FZ_LD];   // working matrix, becomes L (block lower triangle)
    __shared__ __attribute__((aligned(16))) double Xs[64 * FZ_LD];   // L^-1
    __shared__ __attribute__((aligned(16))) double Ts[16 * FZ_LD];   // one scratch tile
    const int lane = threadIdx.x, r = lane & 15, q = lane >> 4;
    const int nb = (f + 15) >> 4;
#pragma unroll 16
    for (int i = 0; i < 64; ++i) {                                   // row i, column `lane`: 16 independent loads in flight
        const int j = lane;
        double v = (i == j) ? 1.0 : 0.0;                             // identity padding for rows / columns >= f
        const double gv = G[min(i, f - 1) * f + min(j, f - 1)];
        if (i < f && j < f) v = gv + (i == j ? lambda : 0.0);
        Gs[i * FZ_LD + j] = v;
        Xs[i * FZ_LD + j] = 0.0;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    int fail = 0;                                                    // first leading minor that is not positive definite
    auto tile = [&](double* M, int bi, int bj) { return M + (16 * bi) * FZ_LD + 16 * bj; };
    auto sync = [&]() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); };
    for (int p = 0; p < nb; ++p) {
        const int bad = fz_diag(tile(Gs, p, p), tile(Gs, p, p), tile(Xs, p, p), FZ_LD, lane);   // in place: row i is read before it is written
        if (bad && !fail) fail = 16 * p + bad;
        sync();
        for (int i = p + 1; i < nb; ++i) {                           // L_ip = G_ip . (L_pp^-1)^T
            const f64x4 c = fz_mul_abt(tile(Gs, i, p), FZ_LD, tile(Xs, p, p), FZ_LD, f64x4{0.0, 0.0, 0.0, 0.0}, r, q, 1.0);
            sync();
            fz_store(tile(Gs, i, p), FZ_LD, c, r, q);
            sync();
        }
        for (int i = p + 1; i < nb; ++i)                             // G_ij -= L_ip . L_jp^T,  p < j <= i
            for (int j = p + 1; j <= i; ++j) {
                const f64x4 c = fz_mul_abt(tile(Gs, i, p), FZ_LD, tile(Gs, j, p), FZ_LD, fz_load(tile(Gs, i, j), FZ_LD, r, q), r, q, -1.0);
                fz_store(tile(Gs, i, j), FZ_LD, c, r, q);
            }
        sync();
    }
    // block forward substitution: X_ip = -X_ii . sum_{k = p .. i-1} L_ik X_kp
    for (int p = 0; p < nb; ++p)
        for (int i = p + 1; i < nb; ++i) {
            f64x4 sacc = f64x4{0.0, 0.0, 0.0, 0.0};
            for (int k = p; k < i; ++k) sacc = fz_mul_ab(tile(Gs, i, k), FZ_LD, tile(Xs, k, p), FZ_LD, sacc, r, q, 1.0);
            fz_store(Ts, FZ_LD, sacc, r, q);
            sync();
            const f64x4 c = fz_mul_ab(tile(Xs, i, i), FZ_LD, Ts, FZ_LD, f64x4{0.0, 0.0, 0.0, 0.0}, r, q, -1.0);
            fz_store(tile(Xs, i, p), FZ_LD, c, r, q);
            sync();
        }
    const bool ok = fail == 0;
    if (lane == 0 && !ok) *info = fail;        // sticky: only the caller resets it (a later success must not hide a failure)
    // Wunwhite[i][j] = X[i][j],  Wwhite[j][i] = X[i][j]; padding columns [f, ld) zero
#pragma unroll 8
    for (int i = 0; i < 64; ++i) {
        if (i >= f) break;
        for (int j = lane; j < ld; j += 64) {                        // ld <= 64 here: one pass
            float wu = 0.f, ww = 0.f;
            if (j < f && ok) { wu = (float)Xs[i * FZ_LD + j]; ww = (float)Xs[j * FZ_LD + i]; }
            Wunwhite[i * ld + j] = wu;
            Wwhite[i * ld + j] = ww;
        }
    }
}

// The feature order P a whitening may be computed in (wmf_compose_whitening, WMF_COMPOSE_REVERSED): 0 the
// identity, 1 diag(1, J) -- feature 0 stays first (the border feature of a bias model), features 1 .. f - 1 reversed --, 2 J, all
// f reversed.  Each is its own inverse.
__host__ __device__ __forceinline__ int wmf_perm(int j, int f, int perm) {
    return perm == 0 ? j : perm == 1 ? (j == 0 ? 0 : f - j) : f - 1 - j;
}

// ---- 64 < f <= 272, blocked: the same algorithm with the two images in a global workspace (L2 resident) and the
// independent tile products of each step dealt to the eight waves of one workgroup.  The columns of L^-1 are
// independent of each other, so each wave substitutes its own columns without further barriers.
__global__ __launch_bounds__(512, 1) void factorize_blocked_kernel(const double* __restrict__ G, int f, int ld, double lambda,
                                                                   float* __restrict__ Wwhite, float* __restrict__ Wunwhite,
                                                                   int32_t* __restrict__ info, double* __restrict__ work, int perm) {
    __shared__ __attribute__((aligned(16))) double Ts[8][16 * 18];   // one scratch tile per wave
    __shared__ int bad;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = (f + 15) >> 4, fp = 16 * nb, LD = fp + 2;
    double* A = work;                                                // fp x LD: working matrix, becomes L
    double* X = work + (size_t)fp * LD;                              // fp x LD: L^-1
    if (tid == 0) bad = 0;
    for (int e = tid; e < fp * fp; e += 512) {
        const int i = e / fp, j = e % fp;
        double v = (i == j) ? 1.0 : 0.0;                             // identity padding for rows / columns >= f
        if (i < f && j < f) v = G[i * f + j] + (i == j ? lambda : 0.0);
        A[i * LD + j] = v;
        X[i * LD + j] = 0.0;
    }
    __syncthreads();
    auto tile = [&](double* M, int bi, int bj) { return M + (size_t)(16 * bi) * LD + 16 * bj; };
    for (int p = 0; p < nb; ++p) {
        if (wave == 0) {
            const int fail = fz_diag(tile(A, p, p), tile(A, p, p), tile(X, p, p), LD, lane);
            if (fail && lane == 0 && !bad) bad = 16 * p + fail;          // the first leading minor that is not positive definite
        }
        __syncthreads();
        for (int i = p + 1 + wave; i < nb; i += 8) {                 // L_ip = A_ip . (L_pp^-1)^T, in place
            const f64x4 c = fz_mul_abt(tile(A, i, p), LD, tile(X, p, p), LD, f64x4{0.0, 0.0, 0.0, 0.0}, r, q, 1.0);
            fz_store(tile(A, i, p), LD, c, r, q);
        }
        __syncthreads();
        int t = 0;
        for (int i = p + 1; i < nb; ++i)                             // A_ij -= L_ip . L_jp^T,  p < j <= i
            for (int j = p + 1; j <= i; ++j, ++t) {
                if ((t & 7) != wave) continue;
                const f64x4 c = fz_mul_abt(tile(A, i, p), LD, tile(A, j, p), LD, fz_load(tile(A, i, j), LD, r, q), r, q, -1.0);
                fz_store(tile(A, i, j), LD, c, r, q);
            }
        __syncthreads();
    }
    // X_ip = -X_ii . sum_{k = p .. i-1} L_ik X_kp, column p by wave p mod 8
    double* ts = Ts[wave];
    for (int p = wave; p < nb; p += 8)
        for (int i = p + 1; i < nb; ++i) {
            f64x4 sacc = f64x4{0.0, 0.0, 0.0, 0.0};
            for (int k = p; k < i; ++k) sacc = fz_mul_ab(tile(A, i, k), LD, tile(X, k, p), LD, sacc, r, q, 1.0);
            fz_store(ts, 18, sacc, r, q);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const f64x4 c = fz_mul_ab(tile(X, i, i), LD, ts, 18, f64x4{0.0, 0.0, 0.0, 0.0}, r, q, -1.0);
            fz_store(tile(X, i, p), LD, c, r, q);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    __syncthreads();
    const bool ok = bad == 0;
    if (tid == 0 && !ok) *info = bad;          // sticky: only the caller resets it (a later success must not hide a failure)
    // G was given in the order P (perm != 0): W_unwhite = L^-1 P^T and W_white = P L^-T leave in feature order
    for (int e = tid; e < f * ld; e += 512) {
        const int i = e / ld, j = e % ld;
        float wu = 0.f, ww = 0.f;
        if (j < f && ok) { wu = (float)X[i * LD + wmf_perm(j, f, perm)]; ww = (float)X[j * LD + wmf_perm(i, f, perm)]; }
        Wunwhite[e] = wu;
        Wwhite[e] = ww;
    }
}

int wmf_launch_factorize(const double* G_sum, int f, int ld, double lambda, float* Wwhite, float* Wunwhite,
                         int32_t* info, double* gA, hipStream_t st, int perm) {
    if (f <= 64) {                                   // blocked single-wave version (fp64 MFMA); perm != 0 comes with f >= 97 only
        WmfProfScope ps("factorize64m_kernel", st);
        hipLaunchKernelGGL(factorize64m_kernel, dim3(1), dim3(64), 0, st, G_sum, f, ld, lambda, Wwhite, Wunwhite, info);
        return 0;
    }
    WmfProfScope ps("factorize_blocked_kernel", st);     // blocked workgroup version (fp64 MFMA)
    hipLaunchKernelGGL(factorize_blocked_kernel, dim3(1), dim3(512), 0, st, G_sum, f, ld, lambda, Wwhite, Wunwhite, info, gA, perm);
    return 0;
}

// ------------------------------------------------------------------------------------- transform
// out[row][:] = in~[row][:] . W.  A wave owns 16-row blocks.  Lane (r = l & 15, q = l >> 4) loads
// 16-byte pieces in[row0 + r][16 t + 4 q .. +3]; its element e is the A operand of MFMA step
// (t, e), whose k slot q then means k = 16 t + 4 q + e; the B operand is W[k][16 nb + r] read from
// the LDS copy of W (row stride ldw = 4 mod 8 dwords keeps the two k rows of a 32-lane half on
// different banks).  The sum over k is order independent, so this k permutation is free.
// NB0 / NBW: this launch produces the NBW output blocks starting at block NB0 (all of them when the whole W fits
// LDS; two or three column slices, each with its own launch, when it does not: f > 176).
template <int NFB, bool W_IN_LDS, int NB0 = 0, int NBW = NFB>
__global__ __launch_bounds__(512) void transform_kernel(const float* __restrict__ in, int64_t m, int f, int ld,
                                                        const float* __restrict__ W, int set_col0_one,
                                                        float* __restrict__ out, float* __restrict__ col0_out,
                                                        int64_t nblocks16) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* Wl = reinterpret_cast<float*>(smem_raw);
    constexpr int KP = 16 * NFB;          // padded K (rows of W)
    constexpr int NP = 16 * NBW;          // padded N of this slice (columns 16 NB0 .. of W)
    constexpr int LDW = NP + 4;           // 4 mod 8 since NP is a multiple of 16
    const int tid = threadIdx.x;
    // nz[kb * NFB + nb] != 0 iff the 16 x 16 tile (kb, nb) of W has a non-zero entry.  Both matrices this kernel is
    // used with are triangular (L^-T, L^-1), so 36 of 81 tile products at f = 129 are skipped -- found from the data,
    // any W stays correct.
    __shared__ int nz[NFB * NBW];
    for (int e = tid; e < NFB * NBW; e += 512) nz[e] = 0;
    __syncthreads();
    for (int e = tid; e < KP * LDW; e += 512) {
        const int a = e / LDW, b = e % LDW, col = 16 * NB0 + b;
        const float v = (a < f && b < NP && col < f) ? W[a * ld + col] : 0.f;
        if constexpr (W_IN_LDS) Wl[e] = v;
        if (v != 0.f) nz[(a >> 4) * NBW + (b >> 4)] = 1;              // benign race: every writer stores 1
    }
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2;
    // per k block t: which output blocks have a non-zero tile of W (wave-uniform bit mask, kept in SGPRs)
    unsigned tmask[NFB];
#pragma unroll
    for (int t = 0; t < NFB; ++t) {
        unsigned mk = 0;
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb) mk |= nz[t * NBW + nb] ? (1u << nb) : 0u;
        tmask[t] = __builtin_amdgcn_readfirstlane(mk);
    }
    // A whole 16-row block (all NFB pieces of a lane's row) is requested at once, and the NEXT block of this wave is
    // requested before the MFMAs of the current one start: 2 x NFB 16-byte loads in flight per lane.  (One piece ahead,
    // as before, left a 10 M x 132 transform at 2.8 TB/s: two 1 KB wave loads in flight per wave hide no HBM latency.)
    // Beyond NFB = 11 (the column-sliced launches for f > 176) two blocks of pieces no longer fit the 256 registers of a
    // wave at two waves per SIMD: one block at a time there, all its pieces requested together.
    constexpr bool DBL = NFB <= 11;
    const int64_t stride = (int64_t)gridDim.x * 8;
    auto request = [&](int64_t blk, float4 (&x)[NFB]) {
        const int64_t row = blk * 16 + r;
        const float4* irow = reinterpret_cast<const float4*>(in + (row < m ? row : 0) * (int64_t)ld);   // loads are unconditional
#pragma unroll
        for (int t = 0; t < NFB; ++t) x[t] = irow[min(4 * t + q, nch - 1)];
    };
    auto block = [&](int64_t blk, float4 (&xc)[NFB], float4 (&xn)[NFB]) {
        if constexpr (DBL) { if (blk + stride < nblocks16) request(blk + stride, xn); }
        const int64_t row = blk * 16 + r;
        const bool rok = row < m;
        f32x4 acc[NBW];
#pragma unroll
        for (int nb = 0; nb < NBW; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < NFB; ++t) {
            const int c = 4 * t + q;                 // 16-byte piece index within the row
            const int k0 = 4 * c;
            // Rows past m compute garbage that is never stored (row r of A only reaches output row r), and every piece but
            // the last lies inside the f features, so only the last piece is masked (its load was clamped).
            float xe[4] = {xc[t].x, xc[t].y, xc[t].z, xc[t].w};
            if (t == NFB - 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) if (!(c < nch && k0 + e < f)) xe[e] = 0.f;
            }
            if (t == 0 && set_col0_one && q == 0) {
                // (set_col0_one == 2, the split layout: col0_out holds {last feature, bias} pairs)
                if (rok && col0_out && NB0 == 0) col0_out[set_col0_one == 2 ? 2 * row + 1 : row] = xe[0];
                xe[0] = 1.f;
            }
            unsigned mv = tmask[t];
            asm volatile("" : "+v"(mv));                     // test the bits here: hoisted, the 81 branch conditions spill
            const unsigned mk = __builtin_amdgcn_readfirstlane(mv);
#pragma unroll
            for (int nb = 0; nb < NBW; ++nb) {
                if (!(mk & (1u << nb))) continue;            // wave-uniform: an all-zero tile of W
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = k0 + e;
                    float b;
                    if constexpr (W_IN_LDS) {
                        b = Wl[k * LDW + 16 * nb + r];
                    } else {
                        const int col = 16 * (NB0 + nb) + r;
                        b = (k < f && col < f) ? W[k * ld + col] : 0.f;
                    }
                    acc[nb] = WMF_MFMA16(xe[e], b, acc[nb]);
                }
            }
        }
        // acc[nb][reg] = out[blk*16 + 4q + reg][16 nb + r]
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t orow = blk * 16 + 4 * q + reg;
            if (orow < m) {
                // split layout (set_col0_one == 2): packed body rows of f - 1 floats, feature f - 1 goes to the pairs
                const bool sp = set_col0_one == 2;
                const int wid = sp ? f - 1 : ld;
                float* o = out + orow * (int64_t)wid;
#pragma unroll
                for (int nb = 0; nb < NBW; ++nb) {
                    const int col = 16 * (NB0 + nb) + r;
                    if (col < wid) o[col] = acc[nb][reg];
                    else if (sp && col == f - 1) col0_out[2 * orow] = acc[nb][reg];
                }
            }
        }
    };
    int64_t blk = (int64_t)blockIdx.x * 8 + wv;
    if constexpr (DBL) {
        float4 xa[NFB], xb[NFB];
        if (blk < nblocks16) request(blk, xa);
        while (blk < nblocks16) {
            block(blk, xa, xb);
            blk += stride;
            if (blk >= nblocks16) break;
            block(blk, xb, xa);
            blk += stride;
        }
    } else {
        float4 xa[NFB];
        for (; blk < nblocks16; blk += stride) {
            request(blk, xa);
            block(blk, xa, xa);
        }
    }
}

// The same product with split-bf16 MFMAs for wide factors (f = 97 .. 144), where the f32 MFMAs bound the kernel above (180 of
// them per 16-row block at f = 129 against a 1.3 ms HBM floor for 10 M rows).  W is split ONCE into three bf16 planes, stored
// transposed in LDS (plane p, output column n, k contiguous: the eight k of a lane's 16x16x32 B operand are one ds_read_b128;
// row stride 176 bf16 = 88 dwords: the 16 lanes that share an LDS cycle of a ds_read_b128 -- {0-3, 12-15, 20-27} .. -- then hit
// 64 distinct banks; at 84 dwords three pairs of them collided and the kernel ran at half speed); the rows of `in` are split on
// the fly (a lane's A operand of K chunk c is the two 16-byte pieces 8 c + 2 q, 8 c + 2 q + 1 of its row).  Six MFMAs per
// (32-wide K chunk, output block) whose W tile is not all zero: 25 of 45 pairs for a triangular W at f = 129.
template <int NFB>
__global__ __launch_bounds__(512) void transform6_kernel(const float* __restrict__ in, int64_t m, int f, int ld,
                                                         const float* __restrict__ W, int set_col0_one,
                                                         float* __restrict__ out, float* __restrict__ col0_out,
                                                         int64_t nblocks16) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NP = 16 * NFB;                 // output columns, padded
    constexpr int NKC = (NP + 31) / 32;          // K chunks of 32
    constexpr int KS = 176;                      // bf16 elements per LDS row (>= 32 NKC = 160): 88 dwords, see above
    static_assert(32 * NKC <= KS, "K does not fit the LDS row");
    __bf16* Wt = reinterpret_cast<__bf16*>(smem_raw);             // [3][NP][KS]
    __shared__ int nz[NKC * NFB];
    const int tid = threadIdx.x;
    for (int e = tid; e < NKC * NFB; e += 512) nz[e] = 0;
    __syncthreads();
    // set_col0_one == 3 / 4: the ROLLED whitened coordinates (include/wmf_hip.h) -- whitened feature c lives at position c - 1 and
    // feature 0 at position f - 1: column n of the matrix in LDS is column n + 1 of W when whitening (3), its row k is row k + 1
    // of W when the input is in those coordinates (4, the un-whitening); both mod f
    const bool roll_n = set_col0_one == 3, roll_k = set_col0_one == 4;
    // One item = eight consecutive k of one column n: consecutive threads take consecutive n (each of the eight loads of a wave
    // reads a contiguous stretch of a row of W), the eight loads are independent and unconditional (an element outside W reads
    // W[0] and is replaced by zero), and the eight parts of a plane leave as one 16-byte LDS write.
    typedef __bf16 stage_bf16x8 __attribute__((ext_vector_type(8)));
    stage_bf16x8* Ws = reinterpret_cast<stage_bf16x8*>(Wt);       // 16-byte units, as Wl below
    for (int it = tid; it < NP * (KS / 8); it += 512) {
        const int k8 = it / NP, n = it - k8 * NP;                 // (NP is a constant: no divide)
        // the roll without a test of the mode per element: position + 1, f wraps to 0 (without a roll, position f is outside W)
        const int rn = roll_n ? 1 : 0, rk = roll_k ? 1 : 0;
        const int ns = n + rn == f ? 0 : n + rn;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * k8 + j;
            const int ks = k + rk == f ? 0 : k + rk;
            const bool in_w = k < f && n < f;
            v[j] = W[in_w ? ks * ld + ns : 0];
            if (!in_w) v[j] = 0.f;
        }
        stage_bf16x8 ph, pm, pl;
        bool any = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const __bf16 h = (__bf16)v[j];
            const float r1 = v[j] - (float)h;
            const __bf16 md = (__bf16)r1;
            ph[j] = h; pm[j] = md; pl[j] = (__bf16)(r1 - (float)md);
            any |= v[j] != 0.f;
        }
        const int at = (n * KS + 8 * k8) / 8;
        Ws[at] = ph;
        Ws[NP * KS / 8 + at] = pm;
        Ws[2 * NP * KS / 8 + at] = pl;
        if (any) nz[(k8 >> 2) * NFB + (n >> 4)] = 1;               // benign race: every writer stores 1 (k8 >> 2 < NKC: k < f there)
    }
    __syncthreads();
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);    // (scalar: a wave's block index and its tests are)
    const int r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2;
    unsigned cmask[NKC];                         // per K chunk: output blocks with a non-zero tile of W
#pragma unroll
    for (int c = 0; c < NKC; ++c) {
        unsigned mk = 0;
#pragma unroll
        for (int nb = 0; nb < NFB; ++nb) mk |= nz[c * NFB + nb] ? (1u << nb) : 0u;
        cmask[c] = __builtin_amdgcn_readfirstlane(mk);
    }
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    const bf16x8_t* Wl = reinterpret_cast<const bf16x8_t*>(Wt);    // 16-byte units: element (p, n, k8) at ((p NP + n) KS + 8 k8) / 8
    const int64_t stride = (int64_t)gridDim.x * 8;
    auto request = [&](int64_t blk, float4 (&x)[2 * NKC]) {
        const int64_t row = blk * 16 + r;
        const float4* irow = reinterpret_cast<const float4*>(in + (row < m ? row : 0) * (int64_t)ld);   // loads are unconditional
#pragma unroll
        for (int c = 0; c < NKC; ++c) {
            x[2 * c] = irow[min(8 * c + 2 * q, nch - 1)];
            x[2 * c + 1] = irow[min(8 * c + 2 * q + 1, nch - 1)];
        }
    };
    const bool in_one = set_col0_one >= 1 && set_col0_one <= 3;      // column 0 of the input reads as 1 (whitening of a bias model)
    const bool sp = set_col0_one == 2 || set_col0_one == 3;          // split layout: packed body rows of f - 1 floats + the pairs
    auto block = [&](int64_t blk, float4 (&xc)[2 * NKC]) {
        const int64_t row = blk * 16 + r;
        const bool rok = row < m;
        float bias_of_row = 0.f;                                     // (lanes q = 0: the bias of row blk 16 + r)
        f32x4 acc[NFB];
#pragma unroll
        for (int nb = 0; nb < NFB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NKC; ++c) {
            const int k0 = 32 * c + 8 * q;                       // first k of this lane's eight
            float xe[8] = {xc[2 * c].x, xc[2 * c].y, xc[2 * c].z, xc[2 * c].w, xc[2 * c + 1].x, xc[2 * c + 1].y, xc[2 * c + 1].z, xc[2 * c + 1].w};
            if (32 * c + 32 > f) {                               // only the last chunk(s) can run past the f features (loads were clamped)
#pragma unroll
                for (int e = 0; e < 8; ++e) if (!(k0 + e < f)) xe[e] = 0.f;
            }
            if (c == 0 && in_one && q == 0) {
                if (rok && col0_out) col0_out[sp ? 2 * row + 1 : row] = xe[0];                     // (split layout: the pairs)
                bias_of_row = xe[0];
                xe[0] = 1.f;
            }
            bf16x8_t ah, am, al;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const __bf16 h = (__bf16)xe[e];
                const float r1 = xe[e] - (float)h;
                const __bf16 md = (__bf16)r1;
                ah[e] = h; am[e] = md; al[e] = (__bf16)(r1 - (float)md);
            }
            unsigned mv = cmask[c];
            asm volatile("" : "+v"(mv));                         // test the bits here (hoisted, the branch conditions spill)
            const unsigned mk = __builtin_amdgcn_readfirstlane(mv);
#pragma unroll
            for (int nb = 0; nb < NFB; ++nb) {
                if (!(mk & (1u << nb))) continue;                // wave-uniform: an all-zero 32 x 16 tile of W
                const int at = ((16 * nb + r) * KS + 32 * c + 8 * q) / 8;
                const bf16x8_t bh = Wl[at], bm = Wl[NP * KS / 8 + at], bl = Wl[2 * NP * KS / 8 + at];
                f32x4 cc = acc[nb];
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bh, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, cc, 0, 0, 0);
                acc[nb] = cc;
            }
        }
        // acc[nb][reg] = out[blk*16 + 4q + reg][16 nb + r].  Every output block but the last lies inside the row in every layout
        // (its columns end at 16 (NFB - 1) - 1 < f - 1 <= wid): its store needs no column test; only the last block has columns
        // past `wid` and, in the split layout, feature f - 1 that goes to the pairs.  Only the last block of a launch has rows
        // past m: a full block (wave-uniform test) stores without a row test either -- a straight line but for the last nb.
        // (3) bits 4 nb + 2 (r / 8) + r % 8 of the row's bias replace the last mantissa bit of body positions 8 j, 8 j + 1 (j < 16):
        // the row kernels that hold 8 consecutive features per lane rebuild the bias from the row they gathered instead of fetching
        // the pair (csrc/wmf_iter.hip); the value moves by at most one ulp.  A select, not a branch.
        const int wid = sp ? f - 1 : ld;
        const bool stuff = set_col0_one == 3 && (r & 7) < 2;
        const int stuff_sh = 2 * (r >> 3) + (r & 7);
        auto store_rows = [&](auto full) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t orow = blk * 16 + 4 * q + reg;
                // (3) the bias of the output row, for its bits: it sits in lane 4 q + reg (q = 0 there)
                const unsigned bbits = set_col0_one == 3 ? (unsigned)__builtin_amdgcn_ds_bpermute((4 * q + reg) * 4, __builtin_bit_cast(int, bias_of_row)) : 0u;
                if (decltype(full)::value || orow < m) {
                    float* o = out + orow * (int64_t)wid;
#pragma unroll
                    for (int nb = 0; nb < NFB; ++nb) {
                        const int col = 16 * nb + r;
                        float v = acc[nb][reg];
                        if (16 * nb < 128) {
                            const unsigned vb = __builtin_bit_cast(unsigned, v);
                            v = __builtin_bit_cast(float, stuff ? ((vb & ~1u) | ((bbits >> (4 * nb + stuff_sh)) & 1u)) : vb);
                        }
                        if (nb < NFB - 1 || col < wid) o[col] = v;
                        else if (sp && col == f - 1) col0_out[2 * orow] = v;
                    }
                }
            }
        };
        if (blk * 16 + 16 <= m) store_rows(std::true_type{});
        else store_rows(std::false_type{});
    };
    // one block of pieces at a time (two, as in transform_kernel, spill at 256 registers: the bf16 parts need room).  Two
    // 16-row blocks per trip sharing every B operand read (twelve MFMAs per three ds_read_b128 instead of six) were measured in
    // round 2: 256 registers + 244 bytes of scratch at NFB = 9, 3.9 ms per cfg3 half step against 2.4.  Requesting the next
    // block's pieces into this block's registers chunk by chunk, as soon as each is split (no spill, a block of arithmetic
    // between request and use): 2.25 against 2.06 ms for 10 M rows in the same process -- the two waves of a SIMD already
    // cover each other's wait, and the kernel moves 5.1 TB/s.
    float4 xa[2 * NKC];
    for (int64_t blk = (int64_t)blockIdx.x * 8 + wv; blk < nblocks16; blk += stride) {
        request(blk, xa);
        block(blk, xa);
    }
}

template <int NFB>
static void launch_transform6(const float* in, int64_t m, int f, int ld, const float* W, int set_col0_one, float* out,
                              float* col0_out, int64_t grid, int64_t nblk, hipStream_t st) {
    constexpr size_t lds = (size_t)3 * 16 * NFB * 176 * 2;
    static_assert(lds <= 158 * 1024, "W planes do not fit LDS");
    // The three planes of W leave room for one workgroup per CU, and every workgroup splits W into them before its first block:
    // one workgroup per CU stages W once per launch (the grid-stride loop of the kernel follows the grid).
    if (grid > wmf_cu_count()) grid = wmf_cu_count();
    static const char* nm = wmf_kname("transform6_kernel<%d>", NFB);
    WMF_LAUNCH_LDS(nm, (transform6_kernel<NFB>), lds, dim3((unsigned)grid), dim3(512), lds, st, in, m, f, ld, W, set_col0_one, out,
                   col0_out, nblk);
}

template <int NFB, int NB0, int NBW>
static void launch_transform_slice(const float* in, int64_t m, int f, int ld, const float* W, int set_col0_one, float* out,
                                   float* col0_out, int64_t grid, int64_t nblk, hipStream_t st) {
    constexpr size_t lds = (size_t)16 * NFB * (16 * NBW + 4) * 4;
    static_assert(lds <= 150 * 1024, "slice too wide");
    static const char* nm = wmf_kname("transform_kernel<%d, true, %d, %d>", NFB, NB0, NBW);
    WMF_LAUNCH_LDS(nm, (transform_kernel<NFB, true, NB0, NBW>), lds, dim3((unsigned)grid), dim3(512), lds, st, in, m, f, ld, W,
                   set_col0_one, out, col0_out, nblk);
}

template <int NFB>
static int launch_transform_nfb(const float* in, int64_t m, int f, int ld, const float* W, int set_col0_one, float* out,
                                 float* col0_out, hipStream_t st) {
    constexpr int KP = 16 * NFB, LDW = KP + 4;
    constexpr size_t lds = (size_t)KP * LDW * 4;
    const int64_t nblk = (m + 15) / 16;
    int64_t grid = (nblk + 7) / 8;
    if (grid > 1024) grid = 1024;
    if (grid < 1) grid = 1;
    // wide factors: split-bf16 products.  The f32 kernel below at those widths (WMF_DBG_F32_TRANSFORM, 262144) is compiled into
    // lab builds only.
    constexpr bool WIDE = NFB >= 7 && NFB <= 9;
    if constexpr (WIDE) {
        if (!WMF_LAB_BUILD || !(wmf_debug_flags & WMF_DBG_F32_TRANSFORM)) {
            launch_transform6<NFB>(in, m, f, ld, W, set_col0_one, out, col0_out, grid, nblk, st);
            return WMF_L_OK;
        }
    }
    if constexpr (WIDE && !WMF_LAB_BUILD) {
        // (not reached: every launch took the branch above)
    } else if constexpr (lds <= 150 * 1024) {
        launch_transform_slice<NFB, 0, NFB>(in, m, f, ld, W, set_col0_one, out, col0_out, grid, nblk, st);
    } else if (in != out) {
        // W does not fit LDS (f > 176): two or three column slices of W, one launch each; every launch reads the
        // input again (it may not alias the output) and writes its own output columns
        constexpr int H = (NFB + 1) / 2;
        if constexpr (H <= 8) {
            launch_transform_slice<NFB, 0, H>(in, m, f, ld, W, set_col0_one, out, col0_out, grid, nblk, st);
            launch_transform_slice<NFB, H, NFB - H>(in, m, f, ld, W, set_col0_one, out, col0_out, grid, nblk, st);
        } else {
            launch_transform_slice<NFB, 0, 6>(in, m, f, ld, W, set_col0_one, out, col0_out, grid, nblk, st);
            launch_transform_slice<NFB, 6, 6>(in, m, f, ld, W, set_col0_one, out, col0_out, grid, nblk, st);
            launch_transform_slice<NFB, 12, NFB - 12>(in, m, f, ld, W, set_col0_one, out, col0_out, grid, nblk, st);
        }
    } else {
        static const char* nm = wmf_kname("transform_kernel<%d, false, 0, %d>", NFB, NFB);
        WMF_LAUNCH(nm, (transform_kernel<NFB, false>), dim3((unsigned)grid), dim3(512), 0, st, in, m, f, ld, W,
                   set_col0_one, out, col0_out, nblk);
    }
    return WMF_L_OK;
}

int wmf_launch_transform(const float* in, int64_t m, int f, int ld, const float* W, int set_col0_one, float* out,
                         float* col0_out, hipStream_t st) {
    if (m <= 0) return WMF_L_OK;
    const int nfb = (f + 15) / 16;
    // set_col0_one == 2 inside the kernels: the split layout (wmf_internal.h) -- `out` is the packed body, col0_out the pairs;
    // 3 / 4 (callers' values, wmf_rolled_layout_supported): the rolled coordinates, transform6_kernel only
    if (set_col0_one == 3 || set_col0_one == 4) {
        if (!wmf_rolled_layout(f, ld)) return WMF_L_NO_KERNEL;
    } else {
        set_col0_one = set_col0_one ? (wmf_split_layout(f, ld) ? 2 : 1) : 0;
    }
    if ((set_col0_one == 2 || set_col0_one == 3) && (!col0_out || in == out)) return WMF_L_LAYOUT;
    return wmf_dispatch_nfb<1, 17>(nfb, [&](auto n) { return launch_transform_nfb<decltype(n)::value>(in, m, f, ld, W, set_col0_one, out, col0_out, st); });
}

// --------------------------------------------------------------------------------------- chained
// The whitening of a side that was just solved, straight from its g ("chained whitening"): the factors
// X = g . U are an exact linear image of g, so the next Gramian and the next whitened side are functions of g and two small
// matrices, and the un-whitening pass leaves the training loop.  With a = [g, 1] (bias; a = g without) and T the (f + bias) x f
// matrix whose rows 0 .. f - 1 are U with column 0 zeroed and whose row f is e0^T (T = U without biases):
//   in~ = a . T,   G~ = T^T (a^T a) T,   V = a . (T . W_white),   bias = g . U[:, 0].
// Row p of T and of N_ext belongs to POSITION p of a row of g and column n of N_ext to position n of the whitened row: in rolled
// coordinates position p holds feature p + 1 (f - 1: feature 0) on both sides.
__device__ __forceinline__ double compose_t(const float* __restrict__ U, int f, int ld, int bias, int rolled, int p, int j) {
    if (p >= f) return j == 0 ? 1.0 : 0.0;                                      // the row of the constant one
    if (bias && j == 0) return 0.0;
    const int src = rolled ? (p + 1 == f ? 0 : p + 1) : p;
    return (double)U[src * ld + j];
}
// The three small products (130^3 at cfg3): sixteen lanes per output element, each with every sixteenth term, summed in a fixed
// order -- a thread per element was one dependent chain of 130 loads and took 40 - 50 us per product.
template <class FA, class FB>
__device__ __forceinline__ double compose_dot16(int n, FA a, FB b) {
    double s = 0.0;
#pragma unroll 3
    for (int k = threadIdx.x & 15; k < n; k += 16) s += a(k) * b(k);
#pragma unroll
    for (int off = 8; off; off >>= 1) s += __shfl_xor(s, off, 16);
    return s;
}
// H = G_aug . T, (f + bias) x f
__global__ __launch_bounds__(256) void compose_h_kernel(const double* __restrict__ Gaug, const float* __restrict__ U, int f, int ld,
                                                        int bias, int rolled, double* __restrict__ H) {
    const int f1 = f + (bias ? 1 : 0);
    const int e0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool live = e0 < f1 * f;
    const int e = live ? e0 : 0;                                                // (whole groups of sixteen: all of them shuffle)
    const int p = e / f, j = e - p * f;
    const double s = compose_dot16(f1, [&](int k) { return Gaug[p * f1 + k]; }, [&](int k) { return compose_t(U, f, ld, bias, rolled, k, j); });
    if (live && (threadIdx.x & 15) == 0) H[e] = s;
}
// G~ = T^T . H, f x f; element (i, j) and (j, i) are the same sum (the factorisation reads one triangle)
// (perm != 0: the output is P^T G~ P, element (i, j) the sum of (P i, P j))
__global__ __launch_bounds__(256) void compose_g_kernel(const double* __restrict__ H, const float* __restrict__ U, int f, int ld,
                                                        int bias, int rolled, double* __restrict__ Gt, int perm) {
    const int f1 = f + (bias ? 1 : 0);
    const int e0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool live = e0 < f * f;
    const int e = live ? e0 : 0;
    int i = e / f, j = e - i * f;
    i = wmf_perm(i, f, perm); j = wmf_perm(j, f, perm);
    if (i > j) { const int t = i; i = j; j = t; }
    const double s = compose_dot16(f1, [&](int p) { return compose_t(U, f, ld, bias, rolled, p, i); }, [&](int p) { return H[p * f + j]; });
    if (live && (threadIdx.x & 15) == 0) Gt[e] = s;
}
// N_ext = [T . W_white | U[:, 0]] on an ld-strided image of f + bias rows, columns in the whitened side's positions
__global__ __launch_bounds__(256) void compose_n_kernel(const float* __restrict__ U, const float* __restrict__ Ww, int f, int ld,
                                                        int bias, int rolled, float* __restrict__ N) {
    const int f1 = f + (bias ? 1 : 0);
    const int e0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const bool live = e0 < f1 * ld;
    const int e = live ? e0 : 0;
    const int p = e / ld, n = e - p * ld;
    const int col = n >= f ? 0 : rolled ? (n + 1 == f ? 0 : n + 1) : n;
    double s = compose_dot16(f, [&](int j) { return compose_t(U, f, ld, bias, rolled, p, j); }, [&](int j) { return (double)Ww[j * ld + col]; });
    if (n >= f) s = (n == f && bias && p < f) ? (double)U[(rolled ? (p + 1 == f ? 0 : p + 1) : p) * ld] : 0.0;   // the bias X[:, 0] = g . U[:, 0]; padding
    if (live && (threadIdx.x & 15) == 0) N[e] = (float)s;
}

// scratch: (f + bias) * f + f * f doubles (the Gramian's partial tiles are free by now)
// flags: WMF_COMPOSE_ROLLED | WMF_COMPOSE_REVERSED.  Reversed: the Gramian is factorised in the order P = diag(1, J) (bias) or J,
// and the factorisation's store puts W_white = P L^-T and W_unwhite = L^-1 P^T back in feature order, so compose_n_kernel and every
// later reader are the same code; only the zeros of N_ext move (anti-triangular: DESIGN.md section 5).
int wmf_launch_compose(const double* G_aug, const float* U, int f, int ld, int bias, int flags, double lambda, float* Wwhite,
                       float* Wunwhite, float* N_ext, int32_t* info, double* scratch, double* gA, hipStream_t st) {
    const int f1 = f + (bias ? 1 : 0);
    const int rolled = (flags & WMF_COMPOSE_ROLLED) ? 1 : 0;
    const int perm = !(flags & WMF_COMPOSE_REVERSED) ? 0 : bias ? 1 : 2;
    double* H = scratch;
    double* Gt = scratch + (size_t)f1 * f;
    WMF_LAUNCH("compose_h_kernel", compose_h_kernel, dim3((f1 * f + 15) / 16), dim3(256), 0, st, G_aug, U, f, ld, bias, rolled, H);
    WMF_LAUNCH("compose_g_kernel", compose_g_kernel, dim3((f * f + 15) / 16), dim3(256), 0, st, H, U, f, ld, bias, rolled, Gt, perm);
    wmf_launch_factorize(Gt, f, ld, lambda, Wwhite, Wunwhite, info, gA, st, perm);
    WMF_LAUNCH("compose_n_kernel", compose_n_kernel, dim3((f1 * ld + 15) / 16), dim3(256), 0, st, U, Wwhite, f, ld, bias, rolled, N_ext);
    return WMF_L_OK;
}

// out = a . N_ext in the layout wmf_row_transform(set_col0_one = mode) writes (0: plain, 1: bias to col0_out, 2: split layout,
// 3: split layout in rolled coordinates with the bias bits in the body), a = [g, 1]: transform6_kernel's body with input
// position f read as 1 and the bias of an output row taken from accumulator column f (the last column of N_ext) instead of
// the input.  Tile pairs of N_ext that are all zero are skipped (nz / cmask, as transform6_kernel): a lower- times an upper-
// triangular matrix is dense, 45 pairs at f = 129 + bias; with one of the two whitenings reversed (wmf_launch_compose) it is
// anti-triangular, 33 pairs, and 24 once the short last chunk starts the accumulators instead (short_tail).
// Bytes per row: one row of g read (4 ld), one packed row (4 (f - 1)) and one pair (8) written.
template <int NFB, int MODE>
__global__ __launch_bounds__(512) void chain6_kernel(const float* __restrict__ in, int64_t m, int f, int ld,
                                                     const float* __restrict__ W,
                                                     float* __restrict__ out, float* __restrict__ col0_out,
                                                     int64_t nblocks16) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int NP = 16 * NFB;
    constexpr int NKC = (NP + 31) / 32;
    constexpr int KS = 176;                      // as transform6_kernel: 88 dwords per LDS row
    static_assert(32 * NKC <= KS, "K does not fit the LDS row");
    __bf16* Wt = reinterpret_cast<__bf16*>(smem_raw);             // [3][NP][KS]
    __shared__ int nz[NKC * NFB];
    __shared__ float ntail[2][NP];                                // rows KB, KB + 1 of N_ext in f32 (the short last chunk, below)
    const int tid = threadIdx.x;
    constexpr bool bias = MODE != 0;
    const int f1 = f + (bias ? 1 : 0);                            // rows and columns of N_ext
    // The last K chunk holds f1 - KB live positions.  One or two of them (f1 = 129, 130; 97, 98) are not worth nine tile pairs and
    // the split of eight values: the accumulators START from those rows of N_ext, a[row][KB] N[KB][col] + a[row][KB + 1] N[KB + 1][col]
    // in plain f32 (with biases and two positions the second value is the one: N[f][col] + g[row][f - 1] N[f - 1][col]), and the
    // chunk leaves the matrix pipe.  Nothing here depends on where N_ext has zeros.
    constexpr int KB = 32 * (NKC - 1);
    const bool short_tail = __builtin_amdgcn_readfirstlane(f1 - KB <= 2 ? 1 : 0) != 0;
    for (int e = tid; e < 2 * NP; e += 512) {
        const int k = KB + e / NP, n = e % NP;
        const bool in_w = k < f1 && n < f1;
        const float v = W[in_w ? k * ld + n : 0];
        ntail[e / NP][n] = in_w ? v : 0.f;
    }
    for (int e = tid; e < NKC * NFB; e += 512) nz[e] = 0;
    __syncthreads();
    typedef __bf16 stage_bf16x8 __attribute__((ext_vector_type(8)));
    stage_bf16x8* Ws = reinterpret_cast<stage_bf16x8*>(Wt);
    for (int it = tid; it < NP * (KS / 8); it += 512) {
        const int k8 = it / NP, n = it - k8 * NP;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * k8 + j;
            const bool in_w = k < f1 && n < f1;
            v[j] = W[in_w ? k * ld + n : 0];
            if (!in_w) v[j] = 0.f;
        }
        stage_bf16x8 ph, pm, pl;
        bool any = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const __bf16 h = (__bf16)v[j];
            const float r1 = v[j] - (float)h;
            const __bf16 md = (__bf16)r1;
            ph[j] = h; pm[j] = md; pl[j] = (__bf16)(r1 - (float)md);
            any |= v[j] != 0.f;
        }
        const int at = (n * KS + 8 * k8) / 8;
        Ws[at] = ph;
        Ws[NP * KS / 8 + at] = pm;
        Ws[2 * NP * KS / 8 + at] = pl;
        if (any) nz[(k8 >> 2) * NFB + (n >> 4)] = 1;               // benign race: every writer stores 1 (k8 >> 2 < NKC: k < f1 there)
    }
    __syncthreads();
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int nch = ld >> 2;
    unsigned cmask[NKC];
#pragma unroll
    for (int c = 0; c < NKC; ++c) {
        unsigned mk = 0;
#pragma unroll
        for (int nb = 0; nb < NFB; ++nb) mk |= nz[c * NFB + nb] ? (1u << nb) : 0u;
        cmask[c] = __builtin_amdgcn_readfirstlane(mk);
    }
    typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
    const bf16x8_t* Wl = reinterpret_cast<const bf16x8_t*>(Wt);
    const int64_t stride = (int64_t)gridDim.x * 8;
    auto request = [&](int64_t blk, float4 (&x)[2 * NKC]) {
        const int64_t row = blk * 16 + r;
        const float4* irow = reinterpret_cast<const float4*>(in + (row < m ? row : 0) * (int64_t)ld);   // loads are unconditional
#pragma unroll
        for (int c = 0; c < NKC; ++c) {
            x[2 * c] = irow[min(8 * c + 2 * q, nch - 1)];
            x[2 * c + 1] = irow[min(8 * c + 2 * q + 1, nch - 1)];
        }
    };
    constexpr bool sp = MODE == 2 || MODE == 3;                         // split layout: packed body rows of f - 1 floats + the pairs
    const int fcol = f & 15;                                         // accumulator column f (the bias) is column fcol of block NFB - 1
    auto block = [&](int64_t blk, float4 (&xc)[2 * NKC]) {
        f32x4 acc[NFB];
        if (short_tail) {
            // positions KB, KB + 1 of row blk 16 + r are in the lanes q = 0 (a solved feature, the one, or nothing: replaced, as
            // below); output row 4 q + reg takes them from lane 4 q + reg
            const float4 xt = xc[2 * (NKC - 1)];
            const float v0 = KB < f ? xt.x : (bias && KB == f) ? 1.f : 0.f;
            const float v1 = KB + 1 < f ? xt.y : (bias && KB + 1 == f) ? 1.f : 0.f;
            float a0[4], a1[4];
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                a0[reg] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((4 * q + reg) * 4, __builtin_bit_cast(int, v0)));
                a1[reg] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((4 * q + reg) * 4, __builtin_bit_cast(int, v1)));
            }
#pragma unroll
            for (int nb = 0; nb < NFB; ++nb) {
                const float n0 = ntail[0][16 * nb + r], n1 = ntail[1][16 * nb + r];
                acc[nb] = f32x4{__builtin_fmaf(a0[0], n0, a1[0] * n1), __builtin_fmaf(a0[1], n0, a1[1] * n1),
                                __builtin_fmaf(a0[2], n0, a1[2] * n1), __builtin_fmaf(a0[3], n0, a1[3] * n1)};
            }
        } else {
#pragma unroll
            for (int nb = 0; nb < NFB; ++nb) acc[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int c = 0; c < NKC; ++c) {
            if (c == NKC - 1 && short_tail) break;                // (wave-uniform)
            const int k0 = 32 * c + 8 * q;
            float xe[8] = {xc[2 * c].x, xc[2 * c].y, xc[2 * c].z, xc[2 * c].w, xc[2 * c + 1].x, xc[2 * c + 1].y, xc[2 * c + 1].z, xc[2 * c + 1].w};
            // f >= 16 (NFB - 1) in every launch: only the last chunk can hold positions past the f solved features -- the one,
            // then nothing (g's padding columns are not trusted: replaced, not multiplied)
            if (32 * c + 32 > 16 * (NFB - 1)) {                  // (a constant once the chunk loop is unrolled)
#pragma unroll
                for (int e = 0; e < 8; ++e) if (!(k0 + e < f)) xe[e] = (bias && k0 + e == f) ? 1.f : 0.f;
            }
            bf16x8_t ah, am, al;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const __bf16 h = (__bf16)xe[e];
                const float r1 = xe[e] - (float)h;
                const __bf16 md = (__bf16)r1;
                ah[e] = h; am[e] = md; al[e] = (__bf16)(r1 - (float)md);
            }
            unsigned mv = cmask[c];
            asm volatile("" : "+v"(mv));
            const unsigned mk = __builtin_amdgcn_readfirstlane(mv);
#pragma unroll
            for (int nb = 0; nb < NFB; ++nb) {
                if (!(mk & (1u << nb))) continue;
                const int at = ((16 * nb + r) * KS + 32 * c + 8 * q) / 8;
                const bf16x8_t bh = Wl[at], bm = Wl[NP * KS / 8 + at], bl = Wl[2 * NP * KS / 8 + at];
                f32x4 cc = acc[nb];
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bm, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(am, bh, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bm, cc, 0, 0, 0);
                cc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, cc, 0, 0, 0);
                acc[nb] = cc;
            }
        }
        // acc[nb][reg] = out[blk*16 + 4q + reg][16 nb + r]; the stores are transform6_kernel's, but the bias of output row
        // 4 q + reg is acc[NFB - 1][reg] of lane 16 q + fcol, and the padding columns [f, ld) of a plain row are written as zero
        const int wid = sp ? f - 1 : ld;
        const bool stuff = MODE == 3 && (r & 7) < 2;
        const int stuff_sh = 2 * (r >> 3) + (r & 7);
        auto store_rows = [&](auto full) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t orow = blk * 16 + 4 * q + reg;
                const float bias_src = acc[NFB - 1][reg];        // (a copy: a bit cast of the vector element itself reads element 0)
                const unsigned bbits = MODE == 3 ? (unsigned)__builtin_amdgcn_ds_bpermute((16 * q + fcol) * 4, __builtin_bit_cast(int, bias_src)) : 0u;
                if (decltype(full)::value || orow < m) {
                    float* o = out + orow * (int64_t)wid;
#pragma unroll
                    for (int nb = 0; nb < NFB; ++nb) {
                        const int col = 16 * nb + r;
                        float v = acc[nb][reg];
                        if (MODE == 3 && 16 * nb < 128) {
                            const unsigned vb = __builtin_bit_cast(unsigned, v);
                            v = __builtin_bit_cast(float, stuff ? ((vb & ~1u) | ((bbits >> (4 * nb + stuff_sh)) & 1u)) : vb);
                        }
                        if (nb < NFB - 1) { o[col] = v; continue; }
                        if (col < wid) o[col] = col < f ? v : 0.f;
                        else if (sp && col == f - 1) col0_out[2 * orow] = v;
                        if (bias && col == f) col0_out[sp ? 2 * orow + 1 : orow] = v;
                    }
                }
            }
        };
        if (blk * 16 + 16 <= m) store_rows(std::true_type{});
        else store_rows(std::false_type{});
    };
    float4 xa[2 * NKC];
    for (int64_t blk = (int64_t)blockIdx.x * 8 + wv; blk < nblocks16; blk += stride) {
        request(blk, xa);
        block(blk, xa);
    }
}

int wmf_launch_transform_chained(const float* g, int64_t m, int f, int ld, int bias, const float* N_ext, int rolled, float* out,
                                 float* col0_out, hipStream_t st) {
    if (m <= 0) return WMF_L_OK;
    const int f1 = f + (bias ? 1 : 0), nfb = (f1 + 15) / 16;
    if (nfb < 7 || nfb > 9) return WMF_L_NO_KERNEL;
    if (rolled && !(bias && wmf_rolled_layout(f, ld))) return WMF_L_NO_KERNEL;
    const int mode = !bias ? 0 : rolled ? 3 : wmf_split_layout(f, ld) ? 2 : 1;          // the layout wmf_row_transform would write
    if (bias && !col0_out) return WMF_L_LAYOUT;
    if (g == out && mode >= 2) return WMF_L_LAYOUT;
    const int64_t nblk = (m + 15) / 16;
    int64_t grid = (nblk + 7) / 8;
    if (grid > wmf_cu_count()) grid = wmf_cu_count();              // one workgroup per CU stages N_ext once (launch_transform6)
    if (grid < 1) grid = 1;
    return wmf_dispatch_nfb<7, 9>(nfb, [&](auto n) {
        constexpr int NFB = decltype(n)::value;
        return wmf_dispatch_nfb<0, 3>(mode, [&](auto md) {
            constexpr int MODE = decltype(md)::value;
            constexpr size_t lds = (size_t)3 * 16 * NFB * 176 * 2;
            static const char* nm = wmf_kname("chain6_kernel<%d, %d>", NFB, MODE);
            WMF_LAUNCH_LDS(nm, (chain6_kernel<NFB, MODE>), lds, dim3((unsigned)grid), dim3(512), lds, st, g, m, f, ld, N_ext, out,
                           col0_out, nblk);
            return (int)WMF_L_OK;
        });
    });
}
