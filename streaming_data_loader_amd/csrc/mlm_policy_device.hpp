// What the kernels that mask a row under a BERT policy (sdl_config.mask_policy 1 / 2; DESIGN.md §3
// "Masking policies") share as code: the Philox RNG contract, the k-smallest select, the wave as
// mlm_pick.hpp asks for it, the row's budget and the 80/10/10 thresholds.  The kernels are the
// unpaired rows (rows_device.hpp row_policy_one), the NSP / SOP pair rows (pair_mlm.hip), the
// packed rows (pack_mlm.hip) and the packed rows over byte-level BPE (pack_mlm_bpe.hip).
//
// The candidates, the pick (keys, policy-1 select, whole-word unit build) and the replacement draws
// are NOT here: they stand in each of the four callers, copied, and a change to one is made to all
// four.  Moved into force-inlined helpers (any one of them alone, with value, reference or scalar
// parameters) they compile to other instruction streams than the copies do, the unpaired and the
// packed rows stages measured 1-3 % slower and a flush kernel gained scratch (DESIGN.md §4 "One
// policy text").  What is here compiles to the callers' code as it was, instruction for instruction.
//
// Row layout (k_rows'): lane L owns positions 256 m + 4 L + w (w = 0..3) of MR rounds m, so one
// Philox block (4 words) is exactly one lane's keys for round m.
#pragma once
#include "device_util.hpp"
#include "kernels.hpp"
#include "mlm_pick.hpp"

namespace sdl {

// ---------------------------------------------------------------------------
// RNG contract: Philox4x32-10 (Salmon et al., SC'11), as oracle/sdl_oracle.c.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// Marks the k smallest (key, position) pairs of a row held as key[m][w]: a
// radix select of the k-th smallest key with wave ballots, then a
// position-ordered tie-break among keys equal to it.  The descent stops as soon
// as exactly k keys lie below the candidate (after ~log2(S) + 2 of the 32
// steps for distinct keys), which selects the same set.
template <int MR>
__device__ __forceinline__ void select_k_smallest(const uint32_t (&key)[MR][4], int k, bool (&sel)[MR][4]) {
    if (k <= 0) {
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) sel[m][w] = false;
        return;
    }
    uint32_t prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = prefix | (1u << bit);
        int c = 0;
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) c += __popcll(__ballot(key[m][w] < cand));
        if (c == k) {  // exactly the k smallest keys lie below cand: no tie to break
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int w = 0; w < 4; ++w) sel[m][w] = key[m][w] < cand;
            return;
        }
        if (c < k) prefix = cand;
    }
    int c_lt = 0;
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) c_lt += __popcll(__ballot(key[m][w] < prefix));
    const int need = k - c_lt;
    const uint64_t lt_mask = (1ull << lane_id()) - 1ull;
    int before = 0;  // equal keys in earlier rounds
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        uint64_t eq[4];
        int lower = 0;  // equal keys of this round in lower lanes
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            eq[w] = __ballot(key[m][w] == prefix);
            lower += __popcll(eq[w] & lt_mask);
        }
        int own = 0;  // equal keys of this lane at lower w
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const bool e = key[m][w] == prefix;
            sel[m][w] = key[m][w] < prefix || (e && before + lower + own < need);
            own += e ? 1 : 0;
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) before += __popcll(eq[w]);
    }
}

// The same selection, usually in far fewer steps: the Philox keys are uniform,
// so an interpolation search over the key range (the next threshold guessed
// from the counts at the bracket's ends) lands on a threshold with exactly k
// keys below it in ~3-4 counts instead of the radix descent's ~log2(S) + 2.
// Any threshold with exactly k keys below it marks the same k-smallest set; a
// tie at the k-th key (no such threshold) or a slow bracket falls back to the
// radix select.
constexpr int ROWS_INTERP_STEPS = 8;
template <int MR>
__device__ __forceinline__ void select_k_smallest_interp(const uint32_t (&key)[MR][4], int k, int nvalid,
                                                         bool (&sel)[MR][4]) {
    if (k > 0 && k < nvalid) {
        uint32_t lo = 0, hi = 0xFFFFFFFFu;  // count(key < lo) = c_lo < k < c_hi ~ count(key < hi)
        int c_lo = 0, c_hi = nvalid;
#pragma unroll 1
        for (int it = 0; it < ROWS_INTERP_STEPS && hi - lo > 1u; ++it) {
            const float f = ((float)(k - c_lo) + 0.5f) / (float)(c_hi - c_lo);
            uint32_t cand = lo + (uint32_t)((float)(hi - lo) * f);
            cand = cand <= lo ? lo + 1u : cand >= hi ? hi - 1u : cand;
            cand = __builtin_amdgcn_readfirstlane(cand);
            int c = 0;
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int w = 0; w < 4; ++w) c += __popcll(__ballot(key[m][w] < cand));
            if (c == k) {
#pragma unroll
                for (int m = 0; m < MR; ++m)
#pragma unroll
                    for (int w = 0; w < 4; ++w) sel[m][w] = key[m][w] < cand;
                return;
            }
            if (c < k) {
                lo = cand;
                c_lo = c;
            } else {
                hi = cand;
                c_hi = c;
            }
        }
    }
    select_k_smallest<MR>(key, k, sel);
}

__device__ __forceinline__ uint32_t max_u32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t min_u32r(uint32_t a, uint32_t b) { return a < b ? a : b; }
// the wave, as mlm_pick.hpp asks for it: sums and minima over all lanes, uniform
struct PickWave {
    uint32_t l;
    __device__ __forceinline__ uint32_t sum(uint32_t x) const {
        return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_sum(x), 63);
    }
    __device__ __forceinline__ uint32_t min(uint32_t x) const {
        DPP_SCAN_ID(x, min_u32r, 0xFFFFFFFFu);
        return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    }
    __device__ __forceinline__ uint32_t lane() const { return l; }
};

// The replacement draw u of a picked position: below MASK_BELOW (80 %) it becomes mask_id, below
// RANDOM_BELOW (10 %) a random id, else (10 %) it stays -- tests/mlm_policy_model.py's MASK_BELOW /
// RANDOM_BELOW.
constexpr uint32_t POLICY_MASK_BELOW = 0xCCCCCCCDu, POLICY_RANDOM_BELOW = 0xE6666667u;

// The row's budget of predictions: per_mille of its l filled positions, rounded; at least 1, at
// most mask_length; none for a row without candidates.
__device__ __forceinline__ int policy_budget(int l, int ncand, int per_mille, int mask_length) {
    int kb = (int)(((int64_t)l * per_mille + 500) / 1000);
    kb = kb < 1 ? 1 : kb;
    kb = kb < mask_length ? kb : mask_length;
    if (ncand == 0) kb = 0;
    return kb;
}

}  // namespace sdl
