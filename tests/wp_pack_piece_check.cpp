// Host check of the chunk list taken by piece against a naive walk over the stage slots
// (csrc/wp_pack.hpp).  What the kernel runs: a chunk without exceptions is gathered through its
// piece descriptors (wp_pair_slots, stale descriptors included), and its test for that -- total
// equal to the piece count, then no bit in any lane's 16 -- must hold exactly for those chunks.
// What it does not run, kept here as the checked statement of where a piece lands (the scatter by
// piece measured slower than packing slot by slot and is not in the kernel): piece number pi at
// slot prel lands at pi + D(prel), D = further-id bits minus no-id bits of the exception bitmap
// below prel; a lane splits its 16 exception bits with its own piece-start mask, and its
// {base, valid mask} record places every piece that starts in its slots.  Built and run by
// tests/test_wp_pack_piece.py.
#include "wp_pack.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace sdl;

// the by-piece placement of a chunk with exceptions (not part of wp_pack.hpp: no kernel calls it)
static uint32_t wp_further_bits(uint32_t vx16, uint32_t starts16) { return vx16 & ~starts16; }
static uint32_t wp_noid_bits(uint32_t vx16, uint32_t starts16) { return vx16 & starts16; }
static int wp_lane_shift(uint32_t vx16, uint32_t starts16) {
    return __builtin_popcount(wp_further_bits(vx16, starts16)) - __builtin_popcount(wp_noid_bits(vx16, starts16));
}
static uint32_t wp_lane_record(uint32_t base, uint32_t valid) { return base | (valid << 16); }
static int wp_record_lane(int prel) { return prel >> 4; }
static bool wp_piece_has_id(uint32_t rec, int prel) { return ((rec >> (16 + (prel & 15))) & 1u) != 0u; }
static uint32_t wp_piece_pos(uint32_t rec, int prel) { return wp_pos(rec & 0xFFFFu, rec >> 16, prel & 15); }

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            if (fails++ < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                            \
    } while (0)

struct Piece {
    int prel, n;  // stage slot of its first byte, ids (0 .. its bytes)
};

// One chunk from its pieces (ascending, a piece's ids within its own bytes, only the last may
// reach the tail slots).  `stale`: what the descriptor list holds past the last piece.
static void check_chunk(const std::vector<Piece> &pieces, std::mt19937 &rng) {
    std::vector<uint32_t> starts16(WP_LANES, 0u), vx(WP_VX_WORDS, 0u);
    std::vector<uint16_t> stage(WP_SLOTS), desc(WP_MAIN);
    for (auto &s : stage) s = (uint16_t)rng();  // slots without an id hold anything
    for (auto &d : desc) d = (uint16_t)rng();   // ... and so do descriptors past the last piece
    uint16_t next_id = 1;
    bool any_exception = false;
    for (size_t pi = 0; pi < pieces.size(); ++pi) {
        const Piece &p = pieces[pi];
        CHECK(p.prel >= 0 && p.prel < WP_MAIN && p.prel + p.n <= WP_SLOTS);
        starts16[p.prel >> 4] |= 1u << (p.prel & 15);
        desc[pi] = (uint16_t)(p.prel | ((1 + rng() % 3) << 12));  // the kind bits are not the slot's
        for (int k = 0; k < p.n; ++k) stage[p.prel + k] = next_id++;
        const WpRange r = wp_exception_range(p.prel, p.n);
        if (r.hi > r.lo) {
            any_exception = true;
            for (int w = r.lo >> 5; w <= (r.hi - 1) >> 5; ++w) vx[w] |= wp_word_mask(w, r.lo, r.hi);
        }
    }
    // naive: the ids in slot order are 1, 2, 3, ...
    std::vector<uint16_t> want;
    for (int s = 0; s < WP_SLOTS; ++s) {
        const int st = s < WP_MAIN ? (int)((starts16[s >> 4] >> (s & 15)) & 1u) : 0;
        if (st ^ (int)((vx[s >> 5] >> (s & 31)) & 1u)) want.push_back(stage[s]);
    }
    CHECK((int)want.size() == next_id - 1);
    for (size_t k = 0; k < want.size(); ++k) CHECK(want[k] == k + 1);
    // naive D at every slot: further-id bits minus no-id bits below it
    std::vector<int> D(WP_MAIN + 1, 0), before(WP_MAIN + 1, 0);
    for (int s = 0; s < WP_MAIN; ++s) {
        const int st = (int)((starts16[s >> 4] >> (s & 15)) & 1u), x = (int)((vx[s >> 5] >> (s & 31)) & 1u);
        D[s + 1] = D[s] + (x && !st) - (x && st);
        before[s + 1] = before[s] + st;
    }
    // the kernel's wave sum and lane records
    uint32_t vx16[WP_LANES], vmain[WP_LANES], vtail[WP_LANES], ex[WP_LANES], rec[WP_LANES], tot = 0;
    int shift = 0;
    for (int t = 0; t < WP_LANES; ++t) {
        vx16[t] = wp_bits16(vx.data(), 16 * t);
        vmain[t] = starts16[t] ^ vx16[t];
        vtail[t] = t < WP_TAIL_LANES ? wp_bits16(vx.data(), WP_MAIN + 16 * t) : 0u;
        ex[t] = tot;
        tot += wp_lane_counts(vmain[t], vtail[t]);
        rec[t] = wp_lane_record(wp_main_base(ex[t]), vmain[t]);
        // a further id never sits on a piece start, a no-id bit always does
        CHECK((wp_further_bits(vx16[t], starts16[t]) | wp_noid_bits(vx16[t], starts16[t])) == vx16[t]);
        CHECK((wp_further_bits(vx16[t], starts16[t]) & starts16[t]) == 0u);
        CHECK(shift == D[16 * t]);
        CHECK((int)wp_main_base(ex[t]) == before[16 * t] + D[16 * t]);
        shift += wp_lane_shift(vx16[t], starts16[t]);
    }
    const uint32_t total = wp_total(tot);
    CHECK(total == want.size());
    bool vx_any = false;  // the kernel's test for (a): a bit in any lane's main or tail slots
    for (int t = 0; t < WP_LANES; ++t) vx_any = vx_any || (vx16[t] | vtail[t]) != 0u;
    CHECK(vx_any == any_exception);
    // ... behind one compare: a chunk whose total differs from its piece count has exceptions
    if (total != pieces.size()) CHECK(vx_any);
    const bool gathers = total == pieces.size() && !vx_any;
    CHECK(gathers == !any_exception);
    // placement by piece + the further ids by their owners (not the kernel's way, see above)
    std::vector<int> hits(WP_SLOTS, 0);
    std::vector<uint16_t> got(WP_SLOTS, 0);
    auto put = [&](uint32_t pos, uint16_t id) {
        CHECK(pos < total);
        if (pos < (uint32_t)WP_SLOTS) {
            ++hits[pos];
            got[pos] = id;
        }
    };
    for (size_t pi = 0; pi < pieces.size(); ++pi) {
        const int prel = (int)(desc[pi] & 0xFFFu);
        const uint32_t r = rec[wp_record_lane(prel)];
        CHECK(wp_piece_has_id(r, prel) == (pieces[pi].n > 0));
        if (!wp_piece_has_id(r, prel)) continue;
        CHECK((int)wp_piece_pos(r, prel) == (int)pi + D[prel]);
        put(wp_piece_pos(r, prel), stage[prel]);
    }
    for (int t = 0; t < WP_LANES; ++t) {
        for (uint32_t m = wp_further_bits(vx16[t], starts16[t]); m; m &= m - 1) {
            const int i = __builtin_ctz(m);
            put(wp_pos(wp_main_base(ex[t]), vmain[t], i), stage[16 * t + i]);
        }
        for (uint32_t m = vtail[t]; m; m &= m - 1) {
            const int i = __builtin_ctz(m);
            put(wp_pos(wp_tail_base(ex[t], tot), vtail[t], i), stage[WP_MAIN + 16 * t + i]);
        }
    }
    for (uint32_t k = 0; k < total; ++k) CHECK(hits[k] == 1 && got[k] == want[k]);
    // no exception (the kernel's gather): the list through the descriptors, eight entries a lane
    if (!any_exception) {
        CHECK(total == pieces.size());
        for (uint32_t e = 0; e < total; e += 8) {
            for (int j = 0; j < 4; ++j) {
                const uint32_t d2 = (uint32_t)desc[e + 2 * j] | ((uint32_t)desc[e + 2 * j + 1] << 16);
                const uint32_t s2 = wp_pair_slots(d2);
                const uint32_t lo = s2 & 0xFFFFu, hi = s2 >> 16;
                CHECK(lo < (uint32_t)WP_MAIN && hi < (uint32_t)WP_MAIN);  // stale entries too
                if (lo >= (uint32_t)WP_MAIN || hi >= (uint32_t)WP_MAIN) continue;
                if (e + 2 * j < total) CHECK(stage[lo] == want[e + 2 * j]);
                if (e + 2 * j + 1 < total) CHECK(stage[hi] == want[e + 2 * j + 1]);
            }
        }
    }
}

int main() {
    std::mt19937 rng(21);
    // empty; one piece; 1,024 one-byte pieces, all with one id and every third with none
    check_chunk({}, rng);
    check_chunk({{5, 1}}, rng);
    check_chunk({{1023, 1}}, rng);
    {
        std::vector<Piece> a, b;
        for (int s = 0; s < WP_MAIN; ++s) {
            a.push_back({s, 1});
            b.push_back({s, s % 3 ? 1 : 0});
        }
        check_chunk(a, rng);
        check_chunk(b, rng);
    }
    // an exception in slot 0 (only a piece without an id can be one), 15, 16 and 1023
    check_chunk({{0, 0}, {3, 1}, {9, 1}}, rng);
    check_chunk({{0, 1}, {14, 2}, {20, 1}}, rng);
    check_chunk({{0, 1}, {15, 2}, {20, 1}}, rng);
    check_chunk({{2, 1}, {16, 0}, {20, 1}}, rng);
    check_chunk({{2, 1}, {1022, 2}}, rng);
    check_chunk({{2, 1}, {1023, 0}}, rng);
    // two exceptions in one 16-slot group: two words of several ids, and one of none beside one
    check_chunk({{30, 1}, {33, 2}, {36, 3}, {50, 1}}, rng);
    check_chunk({{30, 1}, {33, 0}, {36, 3}, {47, 4}, {70, 1}}, rng);
    // a last word whose ids reach the tail slots: a few, and all of them
    check_chunk({{4, 1}, {1018, 13}}, rng);
    check_chunk({{4, 2}, {1000, 0}, {1023, 100}}, rng);
    check_chunk({{0, WP_SLOTS}}, rng);
    check_chunk({{1023, WP_SLOTS - 1023}}, rng);

    // random chunks: pieces with 0 .. bytes ids, a last word over the chunk's end
    for (int it = 0; it < 4000; ++it) {
        std::vector<Piece> ps;
        const int density = 1 + (int)(rng() % 12);
        const int mode = (int)(rng() % 4);  // 0: no exception at all
        int s = (int)(rng() % 40);
        while (s < WP_MAIN) {
            int len = 1 + (int)(rng() % (2 * density));  // the piece's bytes
            if (rng() % 64 == 0) len += (int)(rng() % 120);
            int room = len;
            if (s + room > WP_SLOTS) room = WP_SLOTS - s;
            int n = 1;
            if (mode && rng() % (mode == 3 ? 2 : 6) == 0) n = (int)(rng() % (unsigned)(room + 1));
            ps.push_back({s, n});
            s += len + (int)(rng() % (unsigned)density);
        }
        check_chunk(ps, rng);
    }
    if (fails) {
        printf("wp_pack_piece: %d failures\n", fails);
        return 1;
    }
    printf("wp_pack_piece ok\n");
    return 0;
}
