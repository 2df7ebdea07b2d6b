// The whole-word pick of the BERT masking policy (DESIGN.md §3 "Masking policies"), without a
// sort.  Includes nothing from HIP, so a host program can run it (tests/test_mlm_policy_model.py
// compiles tests/mlm_pick_check.cpp against it).
//
// The contract visits a row's units in ascending (key, first position) with `left = k` and takes
// a unit iff its size fits what is left -- BERT's skip rule.  The picked set is a fixed point of
// "the longest key-ordered prefix whose sizes fit":
//   1. a unit larger than `left` is never taken (left only shrinks): drop them all;
//   2. if the rest fit together, take them and stop; otherwise the longest prefix of the rest
//      whose sizes sum to <= left is taken unit by unit by the contract's walk (every unit in it
//      fits when it is reached), and the unit after it does not fit what is then left;
//   3. subtract, go on above that unit with step 1 (which drops it).
// Every round takes at least one unit, and after it everything left is smaller than the unit
// that ended it: the rounds are bounded by the distinct unit sizes of the row.
//
// The prefix is found like select_k_smallest_interp finds the k-th key, with sums of sizes in the
// place of counts: an interpolation search over the key range for a bracket [lo, hi) with
// sum(key < lo) <= left < sum(key < hi) that holds exactly one unit -- the one that ends the
// round.  A bracket that cannot be split (two units with one key) or a slow search falls back to
// a radix descent for the largest threshold whose sum fits, and walks the units at that key in
// position order, as the contract's (key, first position) order says.  Two units of a row share
// a key with probability 2^-32 a pair; the keys are Philox words, so no input provokes it: only
// the host test (forced equal keys) covers that walk.
//
// Data layout: a lane holds E elements; element e of lane L is row position
// 256 (e >> 2) + 4 L + (e & 3) (k_rows' layout).  size[e] > 0 marks the first position of a
// live unit.  W gives the wave: sum(x) and min(x) over all lanes (uniform results) and lane().
// On the host a "wave" of one lane holds the whole row.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MLM_PICK_FN __host__ __device__ inline
#else
#define MLM_PICK_FN inline
#endif

namespace sdl {

constexpr int MLM_PICK_INTERP_STEPS = 8;

// key < t for a threshold in [0, 2^32] (uniform: the high word is a scalar test)
MLM_PICK_FN bool mlm_key_below(uint32_t key, uint64_t t) { return (t >> 32) != 0 || key < (uint32_t)t; }

// sum of the live sizes with key < t, and their count << 16 (a row has <= 2048 positions)
template <int E, class W>
MLM_PICK_FN uint32_t mlm_pick_below(const uint32_t (&key)[E], const uint32_t (&size)[E], uint64_t t, const W &wv) {
    uint32_t s = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int e = 0; e < E; ++e) s += mlm_key_below(key[e], t) && size[e] ? size[e] + 0x10000u : 0u;
    return wv.sum(s);
}

// Returns the picked units as a bit per element (bit e: the unit that starts at element e).
// size[] is used up.
template <int E, class W>
MLM_PICK_FN uint32_t mlm_pick_units(const uint32_t (&key)[E], uint32_t (&size)[E], uint32_t k, const W &wv) {
    static_assert(E <= 32, "one bit per element");
    uint32_t taken = 0, left = k;
    auto take_below = [&](uint64_t t) {  // take the live units with key < t
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int e = 0; e < E; ++e)
            if (mlm_key_below(key[e], t) && size[e]) {
                taken |= 1u << e;
                size[e] = 0;
            }
    };
    auto drop_below = [&](uint64_t t) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int e = 0; e < E; ++e)
            if (mlm_key_below(key[e], t)) size[e] = 0;
    };
    while (left > 0) {
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int e = 0; e < E; ++e)
            if (size[e] > left) size[e] = 0;
        const uint32_t all = mlm_pick_below<E>(key, size, 1ull << 32, wv);
        if (all == 0) break;
        if ((all & 0xFFFFu) <= left) {
            take_below(1ull << 32);
            break;
        }
        // sum(key < lo) = s_lo <= left < s_hi = sum(key < hi); c_*: the units counted
        uint64_t lo = 0, hi = 1ull << 32;
        uint32_t s_lo = 0, c_lo = 0, s_hi = all & 0xFFFFu, c_hi = all >> 16;
        bool found = c_hi - c_lo == 1;
        for (int it = 0; !found && it < MLM_PICK_INTERP_STEPS && hi - lo > 1; ++it) {
            const float f = ((float)(left - s_lo) + 0.5f) / (float)(s_hi - s_lo);
            uint64_t cand = lo + (uint64_t)((float)(hi - lo) * f);
            cand = cand <= lo ? lo + 1 : cand >= hi ? hi - 1 : cand;
            const uint32_t b = mlm_pick_below<E>(key, size, cand, wv);
            if ((b & 0xFFFFu) <= left) {
                lo = cand;
                s_lo = b & 0xFFFFu;
                c_lo = b >> 16;
            } else {
                hi = cand;
                s_hi = b & 0xFFFFu;
                c_hi = b >> 16;
            }
            found = c_hi - c_lo == 1;
        }
        if (found) {  // [lo, hi) holds the one unit that no longer fits
            take_below(lo);
            left -= s_lo;
            drop_below(hi);
            continue;
        }
        // the largest t with sum(key < t) <= left; some unit has key t (the sum of all is > left)
        uint32_t t = 0, s_t = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            const uint32_t b = mlm_pick_below<E>(key, size, cand, wv) & 0xFFFFu;
            if (b <= left) {
                t = cand;
                s_t = b;
            }
        }
        take_below(t);
        left -= s_t;
        for (;;) {  // the units at key t, in position order
            uint32_t p = 0xFFFFFFFFu;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int e = E - 1; e >= 0; --e)
                if (key[e] == t && size[e]) p = 256u * (uint32_t)(e >> 2) + 4u * wv.lane() + (uint32_t)(e & 3);
            p = wv.min(p);
            if (p == 0xFFFFFFFFu) break;
            uint32_t mine = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int e = 0; e < E; ++e)
                if (256u * (uint32_t)(e >> 2) + 4u * wv.lane() + (uint32_t)(e & 3) == p) mine = size[e];
            const uint32_t sz = wv.sum(mine);
            const bool fits = sz <= left;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int e = 0; e < E; ++e)
                if (256u * (uint32_t)(e >> 2) + 4u * wv.lane() + (uint32_t)(e & 3) == p && size[e]) {
                    if (fits) taken |= 1u << e;
                    size[e] = 0;
                }
            if (fits) left -= sz;
        }
        drop_below((uint64_t)t + 1);
    }
    return taken;
}

}  // namespace sdl
