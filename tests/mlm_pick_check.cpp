// csrc/mlm_pick.hpp against the contract's own walk (sort the units by (key, first position),
// take what fits), on random sizes and keys: full-range keys (the interpolation search), keys
// from a handful of values (forced ties: the radix fallback and its position-ordered walk) and
// mixtures.  A one-lane "wave" holds the row.  Prints "mlm_pick ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mlm_pick.hpp"

struct OneLane {
    uint32_t sum(uint32_t x) const { return x; }
    uint32_t min(uint32_t x) const { return x; }
    uint32_t lane() const { return 0; }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

template <int E>
static uint32_t model(const uint32_t (&key)[E], const uint32_t (&size)[E], uint32_t k) {
    std::vector<int> u;
    for (int e = 0; e < E; ++e)
        if (size[e]) u.push_back(e);
    // (one lane: the element index orders as the position does)
    std::sort(u.begin(), u.end(), [&](int a, int b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
    uint32_t taken = 0, n = 0;
    for (int e : u) {
        if (n >= k) break;
        if (size[e] > k - n) continue;
        taken |= 1u << e;
        n += size[e];
    }
    return taken;
}

template <int E>
static long run(int cases) {
    long bad = 0;
    for (int c = 0; c < cases; ++c) {
        uint32_t key[E], size[E], work[E];
        const int mode = (int)(rnd() % 4);     // 0 full-range keys, 1 few values, 2 mixed, 3 extremes
        const uint32_t maxsize = 1 + rnd() % 6;
        const uint32_t density = 1 + rnd() % 4;
        for (int e = 0; e < E; ++e) {
            size[e] = rnd() % density == 0 ? 0u : 1 + rnd() % maxsize;
            const uint32_t r = rnd();
            key[e] = mode == 0 ? r * 65536u + rnd() : mode == 1 ? r % 3 : mode == 2 ? (r & 1 ? r % 4 * 0x40000000u : r * 65536u + rnd())
                                                                      : (r % 3 == 0 ? 0u : r % 3 == 1 ? 0xFFFFFFFFu : 0xFFFFFFFEu);
        }
        uint32_t total = 0;
        for (int e = 0; e < E; ++e) total += size[e];
        const uint32_t k = rnd() % (total + 3);
        for (int e = 0; e < E; ++e) work[e] = size[e];
        const uint32_t got = sdl::mlm_pick_units<E>(key, work, k, OneLane{});
        const uint32_t want = model<E>(key, size, k);
        if (got != want) {
            if (bad < 5) std::printf("E=%d case %d mode %d k=%u: got %08x want %08x\n", E, c, mode, k, got, want);
            ++bad;
        }
    }
    return bad;
}

int main() {
    long bad = 0;
    bad += run<4>(20000);
    bad += run<8>(20000);
    bad += run<16>(20000);
    bad += run<32>(20000);
    if (bad) {
        std::printf("mlm_pick: %ld mismatches\n", bad);
        return 1;
    }
    std::printf("mlm_pick ok\n");
    return 0;
}
