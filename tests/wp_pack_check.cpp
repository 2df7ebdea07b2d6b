// Host check of csrc/wp_pack.hpp against naive loops over the stage slots: exception bits of a
// finished piece, packing positions of the valid slots (main then tail) and the id offset of a
// record boundary.  Built and run by tests/test_wp_pack.py.
#include "wp_pack.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace sdl;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) {                                                  \
            if (fails++ < 20) printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
        }                                                            \
    } while (0)

// One chunk: `starts` = piece-start bits of the main slots, `vx` = exception bitmap.  Packs the
// way the kernel does (per lane, from the wave sums) and compares with a walk over all slots.
static void check_chunk(const std::vector<uint32_t> &starts16, const std::vector<uint32_t> &vx,
                        const std::vector<int> &boundaries) {
    // naive: valid[s] for every slot, positions in slot order
    std::vector<int> valid(WP_SLOTS, 0), pos(WP_SLOTS, -1);
    for (int s = 0; s < WP_SLOTS; ++s) {
        const int st = s < WP_MAIN ? (int)((starts16[s >> 4] >> (s & 15)) & 1u) : 0;
        valid[s] = st ^ (int)((vx[s >> 5] >> (s & 31)) & 1u);
    }
    int n = 0;
    for (int s = 0; s < WP_SLOTS; ++s)
        if (valid[s]) pos[s] = n++;
    // the kernel's way
    uint32_t vmain[WP_LANES], vtail[WP_LANES], ex[WP_LANES], tot = 0;
    for (int t = 0; t < WP_LANES; ++t) {
        vmain[t] = starts16[t] ^ wp_bits16(vx.data(), 16 * t);
        vtail[t] = t < WP_TAIL_LANES ? wp_bits16(vx.data(), WP_MAIN + 16 * t) : 0u;
        ex[t] = tot;
        tot += wp_lane_counts(vmain[t], vtail[t]);
    }
    CHECK((int)wp_total(tot) == n);
    std::vector<int> list(WP_SLOTS, -1);  // list position -> slot
    for (int t = 0; t < WP_LANES; ++t) {
        for (int i = 0; i < 16; ++i) {
            if ((vmain[t] >> i) & 1u) {
                const uint32_t p = wp_pos(wp_main_base(ex[t]), vmain[t], i);
                CHECK(p < (uint32_t)n && list[p] < 0);
                if (p < (uint32_t)WP_SLOTS) list[p] = 16 * t + i;
                CHECK((int)p == pos[16 * t + i]);
            }
            if ((vtail[t] >> i) & 1u) {
                const uint32_t p = wp_pos(wp_tail_base(ex[t], tot), vtail[t], i);
                CHECK(p < (uint32_t)n && list[p] < 0);
                if (p < (uint32_t)WP_SLOTS) list[p] = WP_MAIN + 16 * t + i;
                CHECK((int)p == pos[WP_MAIN + 16 * t + i]);
            }
        }
    }
    for (int p = 0; p < n; ++p) CHECK(list[p] >= 0);
    for (int rel : boundaries) {
        int before = 0;
        for (int s = 0; s < rel; ++s) before += valid[s];
        const int l = wp_boundary_lane(rel);
        CHECK(l >= 0 && l < WP_LANES);
        CHECK((int)wp_boundary_offset(wp_main_base(ex[l]), vmain[l], rel) == before);
    }
}

int main() {
    std::mt19937 rng(8);
    const std::vector<int> edge_b = {0, 15, 16, 1023};
    std::vector<uint32_t> starts(WP_LANES, 0u), vx(WP_VX_WORDS, 0u);
    // empty
    check_chunk(starts, vx, edge_b);
    // all 16 bits set in every lane (and, second, the whole tail too)
    for (auto &s : starts) s = 0xFFFFu;
    check_chunk(starts, vx, edge_b);
    for (int w = WP_MAIN / 32; w < WP_VX_WORDS; ++w) vx[w] = ~0u;
    check_chunk(starts, vx, edge_b);
    // only tail slots
    for (auto &s : starts) s = 0u;
    check_chunk(starts, vx, edge_b);
    vx.assign(WP_VX_WORDS, 0u);
    vx[WP_MAIN / 32 + 1] = 0x00010080u;
    check_chunk(starts, vx, edge_b);
    // every id in one lane; one id in the last slot
    vx.assign(WP_VX_WORDS, 0u);
    starts[37] = 0xFFFFu;
    check_chunk(starts, vx, edge_b);
    starts.assign(WP_LANES, 0u);
    starts[63] = 0x8000u;
    check_chunk(starts, vx, edge_b);

    // wp_word_mask / wp_exception_range against bit-by-bit setting
    for (int it = 0; it < 20000; ++it) {
        const int prel = (int)(rng() % WP_MAIN);
        int n = (int)(rng() % 5 == 0 ? rng() % 129 : rng() % 6);
        if (prel + n > WP_SLOTS) n = WP_SLOTS - prel;
        const WpRange r = wp_exception_range(prel, n);
        std::vector<uint32_t> a(WP_VX_WORDS, 0u), b(WP_VX_WORDS, 0u);
        if (n == 0) a[prel >> 5] |= 1u << (prel & 31);
        for (int k = 1; k < n; ++k) a[(prel + k) >> 5] |= 1u << ((prel + k) & 31);
        if (r.hi > r.lo)
            for (int w = r.lo >> 5; w <= (r.hi - 1) >> 5; ++w) b[w] |= wp_word_mask(w, r.lo, r.hi);
        CHECK(r.hi >= r.lo && r.hi <= WP_SLOTS);
        CHECK(a == b);
        for (int w = 0; w < WP_VX_WORDS; ++w) CHECK(wp_word_mask(w, r.lo, r.hi) == a[w]);
    }

    // random chunks built the way the kernel's are: pieces with 0..n ids inside their own bytes
    for (int it = 0; it < 3000; ++it) {
        starts.assign(WP_LANES, 0u);
        vx.assign(WP_VX_WORDS, 0u);
        std::vector<int> bnd = edge_b;
        const int density = 1 + (int)(rng() % 12);
        int s = (int)(rng() % 40);
        while (s < WP_MAIN) {
            const int len = 1 + (int)(rng() % (2 * density));          // the piece's bytes
            int room = len;
            if (s + room > WP_SLOTS) room = WP_SLOTS - s;
            int n = rng() % 4 ? 1 : (int)(rng() % (unsigned)(room + 1));   // its ids: 0 .. bytes
            starts[s >> 4] |= 1u << (s & 15);
            const WpRange r = wp_exception_range(s, n);
            if (r.hi > r.lo)
                for (int w = r.lo >> 5; w <= (r.hi - 1) >> 5; ++w) vx[w] |= wp_word_mask(w, r.lo, r.hi);
            s += len;
            if (rng() % 8 == 0 && s < WP_MAIN) bnd.push_back(s);  // a record boundary ends the piece
            s += (int)(rng() % (unsigned)density);
            if (rng() % 16 == 0 && s < WP_MAIN) bnd.push_back(s);  // ... or lies in the gap
        }
        check_chunk(starts, vx, bnd);
    }
    if (fails) {
        printf("wp_pack: %d failures\n", fails);
        return 1;
    }
    printf("wp_pack ok\n");
    return 0;
}
