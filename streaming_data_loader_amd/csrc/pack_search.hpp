// pack_search.hpp -- stream position -> record, for the packed rows kernels (pack.hip,
// pack_mlm.hip).  pk_off[r] is the stream position where record r starts (an exclusive scan of
// the packed lengths seeded with the carry length); records of length 0 (dropped) share their
// successor's offset and are never the answer.
#pragma once
#include <cstdint>

namespace sdl {

// The record holding stream position p, c0 <= p < L: the last r in [lo, hi] with pk_off[r] <= p.
// The caller guarantees pk_off[lo] <= p.
__device__ __forceinline__ uint32_t pack_record_of(const uint32_t *__restrict__ pk_off, uint32_t lo, uint32_t hi,
                                                   uint32_t p) {
    while (lo < hi) {
        const uint32_t m = lo + (hi - lo + 1u) / 2u;
        if (pk_off[m] <= p) lo = m;
        else hi = m - 1u;
    }
    return lo;
}

// The same for a caller whose answer lies near lo (a lane after its wave's search, or after its
// own last position): a galloping search, one or two loads where a binary search over every
// record takes log2 R dependent ones.
__device__ __forceinline__ uint32_t pack_record_near(const uint32_t *__restrict__ pk_off, uint32_t lo, uint32_t last,
                                                     uint32_t p) {
    uint32_t step = 1u;
    while (lo + step <= last && pk_off[lo + step] <= p) {
        lo += step;
        step <<= 1;
    }
    const uint32_t hi = lo + step - 1u < last ? lo + step - 1u : last;
    return pack_record_of(pk_off, lo, hi, p);
}

}  // namespace sdl
