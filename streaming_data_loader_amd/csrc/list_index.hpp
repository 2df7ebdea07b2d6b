// Index arithmetic of the per-chunk id lists (WordPiece: packed u16, LIST_STRIDE slots a chunk):
// global id index -> (chunk, position in the chunk's list), and the chunks a record's ids can lie
// in.  Includes nothing from HIP, so a host program can call it (tests/test_list_index.py).
//
// chunk_off[0 .. n] is the exclusive scan of the chunks' id counts (chunk_off[n] = the total): id
// t lies in the one chunk c with chunk_off[c] <= t < chunk_off[c + 1], at position
// t - chunk_off[c] of its list.  Chunks without ids repeat their neighbour's offset and are never
// the answer.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LIST_INDEX_FN __host__ __device__ inline
#else
#define LIST_INDEX_FN inline
#endif

namespace sdl {

constexpr int64_t LIST_CHUNK = 1024;            // = CHUNK: text bytes a chunk owns
constexpr int64_t LIST_STRIDE = LIST_CHUNK + 128;  // = STAGE: list slots a chunk

struct ListBracket {
    int64_t lo, hi;  // the record's ids lie in chunks [lo, hi]
};

// A record of bytes [a, b): an id belongs to the chunk that owns its piece's first byte, so the
// record's ids lie in the chunks of its own bytes (b > a; n chunks in all).
LIST_INDEX_FN ListBracket list_bracket(uint64_t a, uint64_t b, int64_t n) {
    ListBracket br;
    br.lo = (int64_t)(a / (uint64_t)LIST_CHUNK);
    br.hi = b > a ? (int64_t)((b - 1) / (uint64_t)LIST_CHUNK) : br.lo;
    if (br.hi > n - 1) br.hi = n - 1;
    if (br.lo > br.hi) br.lo = br.hi;
    return br;
}

// The chunk of id t, known to lie in [lo, hi]: the last c there with chunk_off[c] <= t.
LIST_INDEX_FN int64_t list_chunk_of(const uint32_t *chunk_off, int64_t lo, int64_t hi, uint32_t t) {
    while (lo < hi) {
        const int64_t m = (lo + hi + 1) >> 1;
        if (chunk_off[m] <= t) lo = m; else hi = m - 1;
    }
    return lo;
}

// Slot of id t of chunk c in the lists' array.
LIST_INDEX_FN int64_t list_slot(const uint32_t *chunk_off, int64_t c, uint32_t t) {
    return c * LIST_STRIDE + (int64_t)(t - chunk_off[c]);
}

}  // namespace sdl
