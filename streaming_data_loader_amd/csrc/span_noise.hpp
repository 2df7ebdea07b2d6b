// T5's span corruption (sdl_config.span_policy 1, DESIGN.md §3 "Span policies"): the parts the
// host and the device share.  Includes nothing from HIP, so a host program can run it
// (tests/test_span_noise_model.py compiles tests/span_noise_check.cpp against it).
//
//   1. span_noise_counts / span_noise_table: a row of n ids has t noise ids in m spans.  Host
//      only (one double step); the device reads the table, one word for every n in 0..S.
//   2. span_select_cuts: the k smallest (key, index) pairs of key[0..cnt) -- the m - 1 cuts of a
//      uniformly random composition of t (or of u = n - t) into m parts.  Any threshold with
//      exactly k keys below it marks that set, and the keys are Philox words, so an
//      interpolation search over the key range (select_k_smallest_interp's, rows_device.hpp)
//      finds one in ~3-4 counts.  A tie at the k-th key (no such threshold) or a slow bracket
//      falls back to a radix descent for the largest threshold with at most k keys below it and
//      walks the keys equal to it in index order.  Two keys of a row tie with probability 2^-32
//      a pair, so no input provokes the walk: only the host check (forced equal keys) covers it.
//   3. span_plan_entry: span s of a row, from where its kept and noise ids start, as the 8 bytes
//      the span row writers read.
//
// W gives the wave: lane(), lanes() and the uniform sum(x) / min(x) over all lanes.  Lane L
// looks at elements L, L + lanes(), ...; on the host a "wave" of one lane holds the whole row.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SPAN_NOISE_FN __host__ __device__ inline
#else
#define SPAN_NOISE_FN inline
#endif

namespace sdl {

constexpr int SPAN_NOISE_INTERP_STEPS = 8;
constexpr uint32_t SPAN_NOISE_DOMAIN = 0x50000000u;  // or-ed into the chunk word of the Philox counter
constexpr uint32_t SPAN_KEEP_DOMAIN = 0x60000000u;
constexpr int SPAN_MAX_SENTINELS = 100;  // <extra_id_0..99>

// ---- 1. counts ---------------------------------------------------------------------------------
// t noise ids in m spans for a row of n ids (per_mille in 1..500, mean >= 1.0 and finite)
inline void span_noise_counts(int n, int per_mille, double mean, int *t, int *m) {
    *t = 0;
    *m = 0;
    if (n < 2) return;
    long tt = ((long)n * per_mille + 500) / 1000;
    tt = tt < 1 ? 1 : tt;
    tt = tt > n - 1 ? n - 1 : tt;
    const double q = (double)tt / mean + 0.5;  // <= t + 0.5: the floor fits a long
    long mm = (long)q;                         // (q > 0: truncation is the floor)
    mm = mm < 1 ? 1 : mm;
    mm = mm > tt ? tt : mm;
    mm = mm > n - tt ? n - tt : mm;
    *t = (int)tt;
    *m = (int)mm;
}

// tab[n] = t | m << 16 for n in 0..S (S + 1 words; S <= 65535)
inline void span_noise_table(int S, int per_mille, double mean, uint32_t *tab) {
    for (int n = 0; n <= S; ++n) {
        int t, m;
        span_noise_counts(n, per_mille, mean, &t, &m);
        tab[n] = (uint32_t)t | (uint32_t)m << 16;
    }
}

// ---- 2. cuts -----------------------------------------------------------------------------------
// key < t for a threshold in [0, 2^32]
SPAN_NOISE_FN bool span_key_below(uint32_t key, uint64_t t) { return (t >> 32) != 0 || key < (uint32_t)t; }

template <class W>
SPAN_NOISE_FN uint32_t span_count_below(const uint32_t *key, uint32_t cnt, uint64_t t, const W &wv) {
    uint32_t c = 0;
    for (uint32_t i = wv.lane(); i < cnt; i += wv.lanes()) c += span_key_below(key[i], t) ? 1u : 0u;
    return wv.sum(c);
}

// Element i is selected iff key[i] < thr, or key[i] == thr and i < tie_end.
struct SpanSel {
    uint64_t thr;
    uint32_t tie_end;
};
SPAN_NOISE_FN bool span_selected(const SpanSel &s, uint32_t key, uint32_t i) {
    return span_key_below(key, s.thr) || ((uint64_t)key == s.thr && i < s.tie_end);
}

template <class W>
SPAN_NOISE_FN SpanSel span_select_cuts(const uint32_t *key, uint32_t cnt, uint32_t k, const W &wv) {
    if (k == 0) return SpanSel{0ull, 0u};
    if (k >= cnt) return SpanSel{1ull << 32, 0u};
    uint64_t lo = 0, hi = 1ull << 32;  // count(key < lo) = c_lo < k < c_hi = count(key < hi)
    uint32_t c_lo = 0, c_hi = cnt;
    for (int it = 0; it < SPAN_NOISE_INTERP_STEPS && hi - lo > 1; ++it) {
        const float f = ((float)(k - c_lo) + 0.5f) / (float)(c_hi - c_lo);
        uint64_t cand = lo + (uint64_t)((float)(hi - lo) * f);
        cand = cand <= lo ? lo + 1 : cand >= hi ? hi - 1 : cand;
        const uint32_t c = span_count_below(key, cnt, cand, wv);
        if (c == k) return SpanSel{cand, 0u};
        if (c < k) {
            lo = cand;
            c_lo = c;
        } else {
            hi = cand;
            c_hi = c;
        }
    }
    // the largest t with count(key < t) <= k; some key equals t (count(all) = cnt > k)
    uint32_t t = 0, c_t = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = t | (1u << bit);
        const uint32_t c = span_count_below(key, cnt, cand, wv);
        if (c <= k) {
            t = cand;
            c_t = c;
        }
    }
    uint32_t end = 0;  // one past the (k - c_t)-th index whose key is t
    for (uint32_t need = k - c_t; need > 0; --need) {
        uint32_t p = 0xFFFFFFFFu;
        for (uint32_t i = wv.lane(); i < cnt; i += wv.lanes())
            if (key[i] == t && i >= end && i < p) p = i;
        end = wv.min(p) + 1u;
    }
    return SpanSel{(uint64_t)t, end};
}

// ---- 3. the row plan -----------------------------------------------------------------------------
// Span s of a row: A kept and B noise ids lie before it, it keeps a ids and then drops b.  In the
// row it starts at input position lp = A + s (a kept ids, then its sentinel) and at source id
// ip = A + B; its labels start at B + s = ip - lp + 2 s (the sentinel, then the b noise ids).
struct SpanEntry {
    uint32_t x;  // lp | a << 16
    uint32_t y;  // ip | b << 16
};
SPAN_NOISE_FN SpanEntry span_plan_entry(uint32_t s, uint32_t A, uint32_t a, uint32_t B, uint32_t b) {
    return SpanEntry{(A + s) | a << 16, (A + B) | b << 16};
}

}  // namespace sdl
