// First-piece table of the WordPiece chunk kernel's first probes (tokenize_wordpiece.hip, step
// 4a): a two-choice cuckoo table of 16-byte slots over the vocabulary's non-"##" pieces of at
// most 14 bytes, so that a word's first probe is two 16-byte loads and a four-dword compare
// instead of the general table's four loads (common.hpp: VSlot), and the table stays a quarter
// of an XCD's L2.  Includes nothing from HIP, so assets.cpp builds the table with the functions
// the kernel looks it up with, and a host program can call them (tests/test_wp_first.py).
//
// A slot is four little-endian dwords: the payload's 14 bytes, zero-padded, in dwords 0-2 and
// the low half of dword 3, and the piece's id in the high half of dword 3 (ids are below 65,536:
// the u16 staging).  An empty slot is all zero: a candidate has at least one non-zero byte, so
// it never matches one.  The zero padding fixes the length (no payload holds a zero byte: the
// builder leaves such a piece out), so the hash and the compare need no length term, and "##"
// pieces are not in the table, so neither needs a `cont` term.  Every other piece -- longer
// ones, "##" ones -- is found through the general table only.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WP_FIRST_FN __host__ __device__ inline
#else
#define WP_FIRST_FN inline
#endif

namespace sdl {

constexpr int WF_MAXLEN = 14;           // payload bytes a slot holds
constexpr uint32_t WF_MAX_SLOTS = 1u << 20;  // wf_slot2 takes 20 bits of its product

struct alignas(16) WfSlot {
    uint32_t w[4];
};

// The candidate's four dwords (c3 < 0x10000) to 32 bits.  Two independent multiplies over the
// dwords folded in pairs by a rotate, then one multiply to finish: three multiplies on a path
// two deep, where the general table's hash has seven in a row.  Every lane does all of it
// whatever its word's length.  The seed goes in before the first multiplies: two words that
// share a fold under one seed do not under another (the host retries with the next seed when a
// table does not build).  The hash may be weak at no cost to a lookup, which is exact and always
// two loads.
WP_FIRST_FN uint32_t wf_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
WP_FIRST_FN uint32_t wf_hash(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t seed) {
    const uint32_t a = (c0 ^ wf_rotl(c2, 13) ^ seed) * 0x9E3779B1u;
    const uint32_t b = (c1 ^ wf_rotl(c3, 7) ^ wf_rotl(seed, 16)) * 0x85EBCA6Bu;
    uint32_t f = a ^ wf_rotl(b, 16);
    f ^= f >> 15;
    f *= 0x2C1B3C6Du;
    return f ^ (f >> 16);
}
// the two slots of a hash (mask = slots - 1, slots a power of two <= WF_MAX_SLOTS)
WP_FIRST_FN uint32_t wf_slot1(uint32_t h, uint32_t mask) { return h & mask; }
WP_FIRST_FN uint32_t wf_slot2(uint32_t h, uint32_t mask) { return ((h * 0xD35A2D97u) >> 12) & mask; }

// id of the candidate if the slot holds it, else -1: one OR of three dword differences and the
// low half of the fourth
WP_FIRST_FN int wf_match(uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t c0, uint32_t c1, uint32_t c2,
                         uint32_t c3) {
    const uint32_t d = (s0 ^ c0) | (s1 ^ c1) | (s2 ^ c2) | ((s3 ^ c3) & 0xFFFFu);
    return d == 0u ? (int)(s3 >> 16) : -1;
}
// ... out of the candidate's two slots (already loaded)
WP_FIRST_FN int wf_result(const uint32_t a[4], const uint32_t b[4], uint32_t c0, uint32_t c1, uint32_t c2,
                          uint32_t c3) {
    const int ra = wf_match(a[0], a[1], a[2], a[3], c0, c1, c2, c3);
    const int rb = wf_match(b[0], b[1], b[2], b[3], c0, c1, c2, c3);
    return ra >= 0 ? ra : rb;
}

// ---- host side: packing, building, plain lookup ---------------------------------------------

// The four dwords of a payload of n <= WF_MAXLEN bytes, zero-padded.
WP_FIRST_FN void wf_pack(const uint8_t *payload, int n, uint32_t c[4]) {
    c[0] = c[1] = c[2] = c[3] = 0u;
    for (int k = 0; k < n; ++k) c[k >> 2] |= (uint32_t)payload[k] << (8 * (k & 3));
}
// Whether a payload can stand in a slot: 1 .. WF_MAXLEN bytes, none of them zero.
WP_FIRST_FN bool wf_fits(const uint8_t *payload, int n) {
    if (n < 1 || n > WF_MAXLEN) return false;
    for (int k = 0; k < n; ++k)
        if (payload[k] == 0u) return false;
    return true;
}
WP_FIRST_FN bool wf_empty(const WfSlot &s) { return (s.w[0] | s.w[1] | s.w[2] | s.w[3]) == 0u; }

// Inserts one piece (id < 65,536) into a table of mask + 1 slots; false if the kicks run out
// (the table is then to be rebuilt with another seed or size).
inline bool wf_insert(WfSlot *tab, uint32_t mask, uint32_t seed, const uint8_t *payload, int n, uint32_t id) {
    WfSlot v;
    wf_pack(payload, n, v.w);
    v.w[3] |= id << 16;
    uint32_t pos = wf_slot1(wf_hash(v.w[0], v.w[1], v.w[2], v.w[3] & 0xFFFFu, seed), mask);
    for (int kick = 0; kick < 500; ++kick) {
        if (wf_empty(tab[pos])) {
            tab[pos] = v;
            return true;
        }
        const WfSlot t = tab[pos];  // evict the occupant to its other slot
        tab[pos] = v;
        v = t;
        const uint32_t h = wf_hash(v.w[0], v.w[1], v.w[2], v.w[3] & 0xFFFFu, seed);
        const uint32_t a = wf_slot1(h, mask), b = wf_slot2(h, mask);
        pos = pos == a ? b : a;
    }
    return false;
}
// id of a payload of n bytes (any n), or -1: what the kernel's two loads and wf_result give.
inline int wf_lookup(const WfSlot *tab, uint32_t mask, uint32_t seed, const uint8_t *payload, int n) {
    if (!wf_fits(payload, n)) return -1;
    uint32_t c[4];
    wf_pack(payload, n, c);
    const uint32_t h = wf_hash(c[0], c[1], c[2], c[3], seed);
    return wf_result(tab[wf_slot1(h, mask)].w, tab[wf_slot2(h, mask)].w, c[0], c[1], c[2], c[3]);
}

constexpr uint32_t WF_SEEDS = 8;  // seeds tried at one size before the table is doubled

struct WfPiece {
    const uint8_t *payload;
    int n;
    uint32_t id;
};
// Builds the table over n pieces, every one wf_fits and no payload twice: the smallest power of
// two of slots with load <= 0.45 that builds, seeds 0 .. WF_SEEDS - 1 at each size.
// alloc(slots) returns zeroed storage for that many slots (this header needs no container).
// Returns the mask, or 0 if no table of up to WF_MAX_SLOTS slots builds.
template <class Alloc>
inline uint32_t wf_build(const WfPiece *pieces, uint32_t n, const Alloc &alloc, uint32_t *seed_out, WfSlot **tab_out) {
    uint32_t slots = 64;
    while ((uint64_t)slots * 45u < (uint64_t)n * 100u) slots <<= 1;
    for (; slots <= WF_MAX_SLOTS; slots <<= 1) {
        for (uint32_t seed = 0; seed < WF_SEEDS; ++seed) {
            WfSlot *tab = alloc(slots);
            bool ok = true;
            for (uint32_t i = 0; i < n && ok; ++i)
                ok = wf_insert(tab, slots - 1, seed, pieces[i].payload, pieces[i].n, pieces[i].id);
            if (ok) {
                *seed_out = seed;
                *tab_out = tab;
                return slots - 1;
            }
        }
    }
    return 0;
}

}  // namespace sdl
