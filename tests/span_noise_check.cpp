// csrc/span_noise.hpp on the host, a one-lane "wave" holding the row.  For every n in 1..2048 and
// several (per mille, mean) pairs: the counts against the contract's bounds and their growth with
// n; the two cut selections (every n under two of the pairs, every pair below 200 ids) against a
// sort of the (key, index) pairs, with full-range random keys
// (the interpolation search) and with keys from a handful of values (forced ties: the radix
// fallback and its index-ordered walk, which no Philox input reaches); and the plan entries built
// from the cuts against the row the contract spells out.  Prints "span_noise ok".
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "span_noise.hpp"

struct OneLane {
    uint32_t lane() const { return 0; }
    uint32_t lanes() const { return 1; }
    uint32_t sum(uint32_t x) const { return x; }
    uint32_t min(uint32_t x) const { return x; }
};

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16) * 65536u + (uint32_t)((z ^ (z >> 31)) & 0xFFFFu);
}

static long bad = 0;
static void expect(bool ok, const char *what, int n, int pm, double mean, int mode) {
    if (ok) return;
    if (bad < 10) std::printf("FAIL %s: n=%d per_mille=%d mean=%g mode=%d\n", what, n, pm, mean, mode);
    ++bad;
}

// `total` cut into m parts by the k = m - 1 smallest (key, i) over i in 1..total-1 (key[i - 1])
static std::vector<uint32_t> starts_by_sort(const std::vector<uint32_t> &key, uint32_t k) {
    std::vector<uint32_t> idx(key.size());
    for (uint32_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key[a] != key[b] ? key[a] < key[b] : a < b; });
    idx.resize(k);
    std::sort(idx.begin(), idx.end());
    std::vector<uint32_t> st{0u};
    for (uint32_t i : idx) st.push_back(i + 1u);
    return st;
}

static std::vector<uint32_t> starts_by_select(const std::vector<uint32_t> &key, uint32_t k) {
    const sdl::SpanSel s = sdl::span_select_cuts(key.data(), (uint32_t)key.size(), k, OneLane{});
    std::vector<uint32_t> st{0u};
    for (uint32_t i = 0; i < key.size(); ++i)
        if (sdl::span_selected(s, key[i], i)) st.push_back(i + 1u);
    return st;
}

static void fill_keys(std::vector<uint32_t> &key, int mode) {
    // 0 full-range keys, 1 three values, 2 all equal, 3 half ties and extremes
    const uint32_t same = rnd();
    for (auto &x : key) {
        const uint32_t r = rnd();
        x = mode == 0 ? r : mode == 1 ? (r % 3u) * 0x7FFFFFFFu : mode == 2 ? same
                          : (r & 1u ? (r >> 1) % 4u * 0x55555555u : r);
    }
}

int main() {
    const int pms[] = {1, 50, 100, 150, 300, 500};
    const double means[] = {1.0, 2.0, 3.0, 5.5, 4000.0};
    long rows = 0, tie_rows = 0;
    for (int pm : pms)
        for (double mean : means) {
            int pt = 0, pmm = 0;
            std::vector<uint32_t> tab(2049);
            sdl::span_noise_table(2048, pm, mean, tab.data());
            for (int n = 0; n <= 2048; ++n) {
                int t, m;
                sdl::span_noise_counts(n, pm, mean, &t, &m);
                expect(tab[n] == ((uint32_t)t | (uint32_t)m << 16), "table", n, pm, mean, -1);
                if (n < 2) {
                    expect(t == 0 && m == 0, "n < 2", n, pm, mean, -1);
                    continue;
                }
                const long want_t = std::min<long>(std::max<long>(((long)n * pm + 500) / 1000, 1), n - 1);
                const long want_m = std::min<long>(
                    std::min<long>(std::max<long>(1, (long)std::floor((double)want_t / mean + 0.5)), want_t), n - want_t);
                expect(t == want_t && m == want_m, "counts", n, pm, mean, -1);
                expect(t >= 1 && t <= n - 1 && m >= 1 && m <= t && m <= n - t, "bounds", n, pm, mean, -1);
                expect(t >= pt && m >= pmm && t + m >= pt + pmm, "growth", n, pm, mean, -1);  // the full row is the worst
                pt = t;
                pmm = m;
                if (n < 4) expect(m == 1, "n < 4 takes no selection", n, pm, mean, -1);
                if (m < 2) continue;
                // every n under two pairs (T5's, and one span an id: m = t), every pair below 200 ids;
                // past 200 ids full-range keys and one of the three tied kinds, in turn
                const bool every_n = (pm == 150 && mean == 3.0) || (pm == 100 && mean == 1.0);
                if (!every_n && n >= 200) continue;
                const int u = n - t;
                for (int mode = 0; mode < 4; ++mode) {
                    if (n >= 200 && mode != 0 && mode != 1 + n % 3) continue;
                    std::vector<uint32_t> kn((size_t)t - 1), kk((size_t)u - 1);
                    fill_keys(kn, mode);
                    fill_keys(kk, mode);
                    const std::vector<uint32_t> nb = starts_by_select(kn, (uint32_t)m - 1);
                    const std::vector<uint32_t> ka = starts_by_select(kk, (uint32_t)m - 1);
                    expect(nb == starts_by_sort(kn, (uint32_t)m - 1), "noise cuts", n, pm, mean, mode);
                    expect(ka == starts_by_sort(kk, (uint32_t)m - 1), "keep cuts", n, pm, mean, mode);
                    ++rows;
                    tie_rows += mode != 0;
                    if (nb.size() != (size_t)m || ka.size() != (size_t)m) continue;
                    // the plan against the contract's row: a_0 kept, b_0 noise, a_1, b_1, ...
                    uint32_t in_at = 0, lab_at = 0, src = 0;
                    bool ok = true;
                    for (int s = 0; s < m; ++s) {
                        const uint32_t A = ka[s], a = (s + 1 < m ? ka[s + 1] : (uint32_t)u) - A;
                        const uint32_t B = nb[s], b = (s + 1 < m ? nb[s + 1] : (uint32_t)t) - B;
                        const sdl::SpanEntry e = sdl::span_plan_entry((uint32_t)s, A, a, B, b);
                        const uint32_t lp = e.x & 0xFFFFu, gg = e.x >> 16, ip = e.y & 0xFFFFu, sz = e.y >> 16;
                        ok = ok && a >= 1 && b >= 1 && lp == in_at && gg == a && ip == src && sz == b &&
                             ip - lp + 2u * (uint32_t)s == lab_at;
                        in_at += a + 1;   // the kept ids and the sentinel
                        lab_at += b + 1;  // the sentinel and the noise ids
                        src += a + b;
                    }
                    expect(ok && src == (uint32_t)n && in_at == (uint32_t)(u + m) && lab_at == (uint32_t)(t + m), "plan", n,
                           pm, mean, mode);
                }
            }
        }
    // the selection's own edges: k = 0, k = cnt, one key, the largest key tied
    {
        std::vector<uint32_t> k1{7u}, top(9, 0xFFFFFFFFu), low(9, 0u);
        expect(starts_by_select(k1, 0).size() == 1 && starts_by_select(k1, 1).size() == 2, "k = 0, k = cnt", 0, 0, 0, 0);
        for (uint32_t k = 0; k <= 9; ++k) {
            expect(starts_by_select(top, k) == starts_by_sort(top, k), "largest key tied", 0, 0, 0, (int)k);
            expect(starts_by_select(low, k) == starts_by_sort(low, k), "smallest key tied", 0, 0, 0, (int)k);
        }
    }
    if (bad || rows < 1000 || tie_rows < 500) {
        std::printf("span_noise: %ld failures over %ld rows (%ld with tied keys)\n", bad, rows, tie_rows);
        return 1;
    }
    std::printf("span_noise ok (%ld rows, %ld with tied keys)\n", rows, tie_rows);
    return 0;
}
