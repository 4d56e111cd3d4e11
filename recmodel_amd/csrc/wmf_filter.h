// Which scored items may enter a row's list (gfx950): the one filter of the catalogue top-n scans and THE place where the order of
// its tests is defined.  Every top-n epilogue (wmf_topn.h, wmf_topn_wide.h, wmf_topn_grouped.h) tests, for a key of row b:
//   1. the threshold -- the epilogue's own comparison, against a register or LDS: a key that cannot enter is never looked up;
//   2. the row's own id (SELF)        self_idx[b], the catalogue row that batch position b is; self_idx == NULL: no such row;
//   3. the row's allow mask (MASK)    allow_bits[allow_idx[b]][allow_words] (allow_idx == NULL: mask 0 for every row; allow_idx[b]
//                                     == -1: row b has none): item j passes when bit j & 31 of word j >> 5 is set -- one load;
//   4. the row's sorted seen list     seen_indices[seen_indptr[b] .. seen_indptr[b + 1]), a binary search -- up to twenty loads.
// Tests 2 - 4 are WmfRowEligible::pass, in that order and after the threshold: a masked-out item never enters a buffer or raises a
// threshold, which is why a filtered call returns, bit for bit, what the seen list with the ineligible items appended returns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// What a launch knows about eligibility, filled in by the host and handed to every launcher as one POD (how it reaches a kernel: the
// macros below).  cand_idx is the
// list form's (the scan's GATHER reads it, wmf_scan.h); a kernel dereferences only the pointers its instantiation tests.
struct WmfRowFilter {
    const int64_t* seen_indptr; const int32_t* seen_indices;
    const uint32_t* allow_bits; int64_t allow_words; const int32_t* allow_idx;
    const int32_t* self_idx; const int32_t* cand_idx;
};

// How the filter crosses a launch.  A kernel takes it as its seven fields, every pointer __restrict__ (WMF_FILTER_PARAMS), and puts
// them together again (WMF_FILTER_FROM_PARAMS); a launch site passes WMF_FILTER_ARGS(flt).  Not as one by-value struct: a pointer
// inside a struct argument carries no no-alias promise, and without it the mask instantiations spill more scalar registers (98 -> 100
// in recommend_scan_kernel<9, 2, 4, 1>; as fields: 98) and ran up to 1.3 % slower (profiles/r23_scan_refactor.json, resources).
#define WMF_FILTER_PARAMS                                                                                                        \
    const int64_t* __restrict__ seen_indptr, const int32_t* __restrict__ seen_indices, const uint32_t* __restrict__ allow_bits,  \
        int64_t allow_words, const int32_t* __restrict__ allow_idx, const int32_t* __restrict__ self_idx,                        \
        const int32_t* __restrict__ cand_idx
#define WMF_FILTER_FROM_PARAMS WmfRowFilter{seen_indptr, seen_indices, allow_bits, allow_words, allow_idx, self_idx, cand_idx}
#define WMF_FILTER_ARGS(F) (F).seen_indptr, (F).seen_indices, (F).allow_bits, (F).allow_words, (F).allow_idx, (F).self_idx, (F).cand_idx

// The forms of a call's filter, a template argument of every top-n scan (wmf_recommend.hip, wmf_sample.hip) and the suffix of its
// profile name.  0, none: the whole catalogue, the seen lists only.  1, the mask form: the whole catalogue, an item inserted only where
// the row's allow mask has its bit (the epilogue's MASK).  2, the list form: the positions of cand_idx (n_items of them) instead of the
// catalogue (the scan's GATHER, two stages of 16 TPS ids past the epilogue's LDS), keys and seen lookups by the real id.  All score
// in one arithmetic: a score does not depend on the item's place in a tile, so forms 1 and 2 give the bits of form 0 with the
// ineligible items appended to every seen row.  The entry points refuse a call with both a mask and a list.
static inline int rec_form(const WmfRowFilter& flt) { return flt.cand_idx ? 2 : flt.allow_bits ? 1 : 0; }
static const char* const REC_FORM_NAME[3] = {"", "mask_", "list_"};
static constexpr size_t rec_form_lds(int tps, int form) { return form == 2 ? (size_t)2 * tps * 16 * 4 : 0; }

// A lane's part of the filter: rows u0 + 4 q + reg, reg < 4, of a batch of n_rows.  Fixed-size arrays under compile-time indices
// (reg comes from an unrolled loop), so they stay in registers; self[] is dead without SELF and words[] without MASK.
template <bool SELF, bool MASK>
struct WmfRowEligible {
    const int32_t* __restrict__ seen_indices;
    int64_t lo[4], hi[4];
    int32_t self[4];
    const uint32_t* words[4];

    __device__ __forceinline__ void begin(const WmfRowFilter& f, int64_t u0, int q, int64_t n_rows) {
        seen_indices = f.seen_indices;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            lo[reg] = 0; hi[reg] = 0;
            const int64_t b = u0 + 4 * q + reg;
            if (f.seen_indptr && b < n_rows) { lo[reg] = f.seen_indptr[b]; hi[reg] = f.seen_indptr[b + 1]; }
            if constexpr (SELF) self[reg] = (f.self_idx && b < n_rows) ? f.self_idx[b] : -1;
            if constexpr (MASK) {
                const int32_t g = b < n_rows ? (f.allow_idx ? f.allow_idx[b] : 0) : -1;
                words[reg] = g >= 0 ? f.allow_bits + (int64_t)g * f.allow_words : nullptr;
            }
        }
    }
    // tests 2 - 4 for a key of row u0 + 4 q + reg that has beaten the row's threshold
    __device__ __forceinline__ bool pass(int reg, int64_t item) const {
        bool take = true;
        if constexpr (SELF) take = (int32_t)item != self[reg];
        if constexpr (MASK) {
            if (take && words[reg]) take = (words[reg][item >> 5] >> (item & 31)) & 1u;
        }
        if (take && lo[reg] < hi[reg]) {
            int64_t a = lo[reg], z = hi[reg];
            while (a < z) {                                        // first entry >= item
                const int64_t mid = (a + z) >> 1;
                if (seen_indices[mid] < (int32_t)item) a = mid + 1; else z = mid;
            }
            take = !(a < hi[reg] && seen_indices[a] == (int32_t)item);
        }
        return take;
    }
};
