// The sentence-level draw of MLM sentence pairs (sdl_config.pair 2..4, DESIGN.md §3 "Sentence
// pairs": "MLM rows and the NSP / SOP draw") and the pair row's kept lengths: the parts the host
// and the device share.  Includes nothing from HIP, so a host program can run it
// (tests/test_pair_mlm_model.py compiles tests/pair_draw_check.cpp against it).
//
// Example r of a call over n_pairs examples has global index rec = first_record + r and takes one
// Philox4x32-10 block, counter (0, PAIR_DRAW_DOMAIN, rec lo, rec hi), key (seed lo, seed hi), words
// x, y, z, w:
//   pair 2       first A_r, second B_r, label 0
//   pair 3 NSP   random = x >= 2^31 && n_pairs >= 2; the second segment is B_s with
//                s = j + (j >= r), j = umulhi(y, n_pairs - 1) -- uniform over the other examples of
//                the call -- when random, else B_r; label = random
//   pair 4 SOP   swap = x >= 2^31: first B_r, second A_r; label = swap
// Text range 2q is A_q and 2q + 1 is B_q, as the pair calls lay them out.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PAIR_DRAW_FN __host__ __device__ inline
#else
#define PAIR_DRAW_FN inline
#endif

namespace sdl {

constexpr uint32_t PAIR_DRAW_DOMAIN = 0x70000000u;  // the chunk word of the draw's Philox counter
// sdl_config.pair (SDL_PAIR_* of include/sdl_batcher.h)
constexpr int PAIR_MODE_NONE = 0, PAIR_MODE_ROWS = 1, PAIR_MODE_MLM = 2, PAIR_MODE_MLM_NSP = 3, PAIR_MODE_MLM_SOP = 4;

struct PairWords {
    uint32_t x, y, z, w;
};
// Philox4x32-10 (Salmon et al., SC'11) as rows_device.hpp and oracle/sdl_oracle.c state it, with
// 64-bit products so the host compiles it too
PAIR_DRAW_FN PairWords pair_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return PairWords{c0, c1, c2, c3};
}

struct PairDraw {
    uint32_t first, second;  // the text ranges of the row's first and second segment
    int32_t label;           // next_sentence_label (pair 2, 3) / sentence_order_label (pair 4)
};
// r < n_pairs < 2^31 (so 2 r + 1 fits 32 bits); mode: PAIR_MODE_MLM ..
PAIR_DRAW_FN PairDraw pair_draw(uint64_t seed, uint64_t rec, uint32_t r, uint32_t n_pairs, int mode) {
    PairDraw d{2u * r, 2u * r + 1u, 0};
    if (mode != PAIR_MODE_MLM_NSP && mode != PAIR_MODE_MLM_SOP) return d;
    const PairWords p = pair_philox4x32_10(0u, PAIR_DRAW_DOMAIN, (uint32_t)rec, (uint32_t)(rec >> 32), (uint32_t)seed,
                                           (uint32_t)(seed >> 32));
    const bool high = p.x >= 0x80000000u;
    if (mode == PAIR_MODE_MLM_NSP) {
        if (high && n_pairs >= 2u) {
            const uint32_t j = (uint32_t)(((uint64_t)p.y * (uint64_t)(n_pairs - 1u)) >> 32);
            const uint32_t s = j + (j >= r ? 1u : 0u);
            d.second = 2u * s + 1u;
            d.label = 1;
        }
    } else if (high) {
        d.first = 2u * r + 1u;
        d.second = 2u * r;
        d.label = 1;
    }
    return d;
}

struct PairKeptLengths {
    uint32_t a, b;
};
// tokenizers' TruncationStrategy::LongestFirst (right, stride 0) for n_a + n_b ids into M = S - 3,
// as pair.hip's pair_kept and tests/pair_model.py kept_lengths: the longer side is cut to what the
// shorter leaves, both to halves once the shorter exceeds its half; on a tie the first segment
// counts as the shorter, so the second gets the odd id.
PAIR_DRAW_FN PairKeptLengths pair_kept_lengths(uint32_t na, uint32_t nb, uint32_t M) {
    if ((uint64_t)na + nb <= M) return PairKeptLengths{na, nb};
    uint32_t lo = na < nb ? na : nb, hi = na < nb ? nb : na;
    hi = lo > M ? lo : (lo > M - lo ? lo : M - lo);
    if ((uint64_t)lo + hi > M) {
        lo = M / 2u;
        hi = M / 2u + M % 2u;
    }
    return na <= nb ? PairKeptLengths{lo, hi} : PairKeptLengths{hi, lo};
}

}  // namespace sdl
