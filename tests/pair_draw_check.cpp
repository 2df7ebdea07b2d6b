// csrc/pair_draw.hpp on the host.  Reads queries from standard input, one a line, and answers each
// on a line of its own, so tests/test_pair_mlm_model.py can compare the header with
// tests/pair_mlm_model.py and tests/pair_model.py value for value:
//   D seed rec r n_pairs mode   ->  first second label      (pair_draw)
//   K n_a n_b M                 ->  k_a k_b                 (pair_kept_lengths)
//   W seed rec                  ->  x y z w                 (the draw's Philox block)
// Every draw is also checked against what the contract promises whatever the words are: ranges of
// the call, a foreign second segment never the row's own, a call of one pair never random, labels
// 0 / 1.  Ends with "pair_draw ok" (or the count of broken promises).
#include <cinttypes>
#include <cstdint>
#include <cstdio>

#include "pair_draw.hpp"

int main() {
    char kind;
    long bad = 0;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'D') {
            uint64_t seed, rec;
            uint32_t r, n;
            int mode;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu32 " %" SCNu32 " %d", &seed, &rec, &r, &n, &mode) != 5) return 2;
            const sdl::PairDraw d = sdl::pair_draw(seed, rec, r, n, mode);
            std::printf("%" PRIu32 " %" PRIu32 " %d\n", d.first, d.second, (int)d.label);
            bool ok = d.first < 2u * n && d.second < 2u * n && (d.label == 0 || d.label == 1);
            if (mode == sdl::PAIR_MODE_MLM) ok = ok && d.first == 2u * r && d.second == 2u * r + 1u && d.label == 0;
            if (mode == sdl::PAIR_MODE_MLM_NSP) {
                ok = ok && d.first == 2u * r && (d.second & 1u) == 1u;
                ok = ok && (d.label == 1) == (d.second != 2u * r + 1u);  // random <=> a foreign B
                if (n < 2u) ok = ok && d.label == 0;
            }
            if (mode == sdl::PAIR_MODE_MLM_SOP)
                ok = ok && d.first == (d.label ? 2u * r + 1u : 2u * r) && d.second == (d.label ? 2u * r : 2u * r + 1u);
            if (!ok) ++bad;
        } else if (kind == 'K') {
            uint32_t na, nb, M;
            if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu32, &na, &nb, &M) != 3) return 2;
            const sdl::PairKeptLengths k = sdl::pair_kept_lengths(na, nb, M);
            std::printf("%" PRIu32 " %" PRIu32 "\n", k.a, k.b);
            const uint64_t sum = (uint64_t)na + nb;
            if (k.a > na || k.b > nb || (uint64_t)k.a + k.b != (sum < M ? sum : M)) ++bad;
        } else if (kind == 'W') {
            uint64_t seed, rec;
            if (std::scanf("%" SCNu64 " %" SCNu64, &seed, &rec) != 2) return 2;
            const sdl::PairWords p = sdl::pair_philox4x32_10(0u, sdl::PAIR_DRAW_DOMAIN, (uint32_t)rec, (uint32_t)(rec >> 32),
                                                             (uint32_t)seed, (uint32_t)(seed >> 32));
            std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", p.x, p.y, p.z, p.w);
        } else {
            return 2;
        }
    }
    if (bad) {
        std::printf("pair_draw: %ld broken promises\n", bad);
        return 1;
    }
    std::printf("pair_draw ok\n");
    return 0;
}
