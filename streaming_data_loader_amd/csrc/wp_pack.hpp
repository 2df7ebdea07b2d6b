// Mask arithmetic of the WordPiece chunk kernel's id compaction (tokenize_wordpiece.hip, step 5):
// which stage slots hold an id, where each lands in the chunk's packed list, and the id offset of
// a record boundary.  Includes nothing from HIP, so a host program can call it
// (tests/test_wp_pack.py, tests/test_wp_pack_piece.py).
//
// A chunk stages its ids in WP_SLOTS slots, a piece's ids from the slot of its first byte on.
// Lane t of the wave owns the main slots [16t, 16t + 16); lanes 0-7 also own the tail slots
// [WP_MAIN + 16t, WP_MAIN + 16t + 16), which only the chunk's last word can reach.  A slot holds
// an id if its bit is set in `piece starts ^ exceptions`: a piece that finished with one id (nearly
// all) needs no exception, one with n > 1 ids sets the bits of its slots 1 .. n-1, one with none
// sets (so clears) its own.  The list is the valid main slots in order, then the valid tail slots.
// (No text reaches the n == 0 case today: a piece starts at a char whose class is not "removed",
// and such a char's normalized form is never empty, so every finished piece has at least one id
// -- [UNK] if nothing else.  The bit's arithmetic is kept whole and checked on the host.)
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WP_PACK_FN __host__ __device__ inline
#else
#define WP_PACK_FN inline
#endif

namespace sdl {

constexpr int WP_MAIN = 1024;                  // = CHUNK
constexpr int WP_SLOTS = WP_MAIN + 128;        // = STAGE
constexpr int WP_LANES = 64, WP_TAIL_LANES = (WP_SLOTS - WP_MAIN) / 16;
constexpr int WP_VX_WORDS = WP_SLOTS / 32;     // words of the exception bitmap

struct WpRange {
    int lo, hi;  // bits [lo, hi)
};

// The exception bits of a piece staged at slot `prel` that finished with n ids.
WP_PACK_FN WpRange wp_exception_range(int prel, int n) {
    if (n == 1) return WpRange{0, 0};
    if (n == 0) return WpRange{prel, prel + 1};
    return WpRange{prel + 1, prel + n};
}

// The bits of [lo, hi) that lie in 32-bit word w of a bitmap.
WP_PACK_FN uint32_t wp_word_mask(int w, int lo, int hi) {
    const int a = lo > 32 * w ? lo - 32 * w : 0;
    const int b = hi < 32 * w + 32 ? hi - 32 * w : 32;
    if (a >= b) return 0u;
    return (b - a == 32 ? ~0u : (1u << (b - a)) - 1u) << a;
}

// 16 bits of a bitmap from bit `slot0` (a multiple of 16) on.
template <class P>
WP_PACK_FN uint32_t wp_bits16(P bitmap, int slot0) {
    return (bitmap[slot0 >> 5] >> (slot0 & 31)) & 0xFFFFu;
}

// One wave sum serves both slot ranges: a lane adds its main count in the low half and its tail
// count in the high half (the main counts sum to at most 1,024: no carry).
WP_PACK_FN uint32_t wp_lane_counts(uint32_t vmain, uint32_t vtail) {
    return (uint32_t)__builtin_popcount(vmain) | ((uint32_t)__builtin_popcount(vtail) << 16);
}
// ex: the exclusive wave sum of wp_lane_counts before this lane; tot: the sum over the wave.
WP_PACK_FN uint32_t wp_total(uint32_t tot) { return (tot & 0xFFFFu) + (tot >> 16); }
WP_PACK_FN uint32_t wp_main_base(uint32_t ex) { return ex & 0xFFFFu; }
WP_PACK_FN uint32_t wp_tail_base(uint32_t ex, uint32_t tot) { return (tot & 0xFFFFu) + (ex >> 16); }

// List position of the lane's slot i (0..15) if it is valid: the lane's base plus its valid slots below.
WP_PACK_FN uint32_t wp_pos(uint32_t base, uint32_t valid, int i) {
    return base + (uint32_t)__builtin_popcount(valid & ((1u << i) - 1u));
}

// A record boundary at chunk offset rel (0 .. WP_MAIN - 1): ids before it in the list, from the
// main base and the main valid mask of lane wp_boundary_lane(rel).  A piece's ids lie in slots of
// its own bytes and a record boundary ends a word, so the valid slots below rel are exactly the
// ids of the pieces that start before it.
WP_PACK_FN int wp_boundary_lane(int rel) { return rel >> 4; }
WP_PACK_FN uint32_t wp_boundary_offset(uint32_t base, uint32_t valid, int rel) { return wp_pos(base, valid, rel & 15); }

// ---- an exception-free chunk, by piece ----------------------------------------------------------
// The chunk's piece list holds a descriptor a piece in list order, the stage slot of the piece's
// first byte in bits 0-11.  In a chunk without an exception bit piece e's one id is list entry
// e, so the list is a gather through the descriptors, with no walk over the 1,152 slots.  Two
// descriptors a dword -> their slots, each kept below WP_MAIN: an entry at or past the piece
// count holds a stale descriptor (any 12 bits), whose id nobody reads but whose slot must still
// lie inside the stage.
WP_PACK_FN uint32_t wp_pair_slots(uint32_t desc2) { return desc2 & (0x00010001u * (uint32_t)(WP_MAIN - 1)); }

}  // namespace sdl
