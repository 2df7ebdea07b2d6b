// Host check of csrc/wp_extent.hpp: for every piece start of a window, the (length, fast flag,
// keep mask, lower-cased bytes) that the stop / fast-terminator bitmaps give against a byte-wise
// restatement of the rule the WordPiece chunk kernel's word_setup used before the bitmaps (16
// bytes classified per piece, the record bits and the non-ASCII bits looked up per piece).
// Built and run by tests/test_wp_extent.py.
#include "wp_extent.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

using namespace sdl;

static int fails = 0;
static long checked = 0;
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            if (fails++ < 20) printf("FAIL %s:%d %s  [%s]\n", __FILE__, __LINE__, #c, what); \
        }                                                                                 \
    } while (0)

constexpr int HALO = 32;                 // right halo bytes of the window
constexpr int SPAN = WX_CHUNK + HALO;    // chunk offsets a window holds

static bool is_alnum(unsigned b) { return (b >= '0' && b <= '9') || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z'); }
static bool is_ws(unsigned b) { return b == ' ' || b == '\t' || b == '\n' || b == '\r'; }
static bool is_iso(unsigned b) { return b >= 32 && b < 127 && !is_alnum(b) && !is_ws(b); }
static unsigned lower(unsigned b) { return b >= 'A' && b <= 'Z' ? b + 32 : b; }

struct Window {
    unsigned char byte[SPAN];   // bytes at or past `n` are zero, as the kernel's loads leave them
    bool rec[SPAN + 1];         // a record starts at the offset
    bool na[WX_CHUNK];          // the rare pass found a non-ASCII whitespace/isolated char (lead bytes only)
    int n;                      // text bytes from the chunk's start on (0 .. SPAN)
    Window() : n(SPAN) {
        memset(byte, 0, sizeof byte);
        memset(rec, 0, sizeof rec);
        memset(na, 0, sizeof na);
    }
    void put(int at, const std::string &s) {
        for (size_t i = 0; i < s.size() && at + (int)i < SPAN; ++i) byte[at + i] = (unsigned char)s[i];
    }
    void cut(int nn) {
        n = nn;
        for (int i = nn; i < SPAN; ++i) byte[i] = 0;
        for (int i = nn; i < WX_CHUNK; ++i) na[i] = false;
    }
};

struct Ref {
    int len;
    bool fast;
    unsigned char kept[16];
};
// The earlier rule, byte by byte.
static Ref ref_setup(const Window &w, int p) {
    int Lw = 0;
    while (Lw < 16 && is_alnum(w.byte[p + Lw])) ++Lw;
    int Lr = 17;
    for (int k = 1; k <= 16; ++k)
        if (w.rec[p + k]) { Lr = k; break; }
    bool fast;
    if (Lr <= Lw) {
        Lw = Lr;
        fast = true;
    } else {
        const unsigned t = w.byte[p + Lw];
        const int te = p + Lw;
        const bool na = t >= 0xC0u && te < WX_CHUNK && w.na[te];
        fast = (t < 0x80u && (is_ws(t) || is_iso(t))) || na || te >= w.n;
    }
    Ref r{Lw, fast, {0}};
    for (int i = 0; i < Lw; ++i) r.kept[i] = (unsigned char)lower(w.byte[p + i]);
    return r;
}

static uint32_t dword(const unsigned char *b) { return b[0] | (b[1] << 8) | (b[2] << 16) | ((uint32_t)b[3] << 24); }

static void check_window(const Window &w, const char *what) {
    // the bitmaps, lane by lane, interleaved as the kernel stores them
    std::vector<uint32_t> sf(2 * WX_WORDS, 0u);
    for (int t = 0; t <= WX_CHUNK / 16; ++t) {  // 64 lanes and the halo piece
        const int s0 = 16 * t;
        uint32_t b[4], rec16 = 0, na16 = 0;
        for (int j = 0; j < 4; ++j) b[j] = dword(w.byte + s0 + 4 * j);
        for (int i = 0; i < 16; ++i) {
            rec16 |= (uint32_t)w.rec[s0 + i] << i;
            if (t < WX_CHUNK / 16) na16 |= (uint32_t)w.na[s0 + i] << i;
        }
        const int nown = w.n <= s0 ? 0 : w.n - s0 < 16 ? w.n - s0 : 16;
        WxStops st = wx_stops(b, rec16, na16, nown);
        // the kernel's two other ways to the same masks: from the classifier's nibbles (its own
        // lanes) and byte by byte (the halo's bytes, by ballot)
        uint32_t nib = 0, an1 = 0, tm1 = 0;
        for (int j = 0; j < 4; ++j) {
            uint32_t n4 = 0;
            for (int i = 0; i < 4; ++i) {
                const unsigned c = w.byte[s0 + 4 * j + i];
                n4 |= (is_alnum(c) ? WX_V_OTHER : is_ws(c) ? WX_V_WS : is_iso(c) ? WX_V_ISO : 0u) << (4 * i);
                an1 |= (uint32_t)wx_is_alnum(c) << (4 * j + i);
                tm1 |= (uint32_t)wx_is_term(c) << (4 * j + i);
            }
            nib |= wx_nibble_classes(n4) << (4 * j);
        }
        const WxStops st2 = wx_stops_from(nib >> 16, nib, rec16, na16, nown), st3 = wx_stops_from(an1, tm1, rec16, na16, nown);
        CHECK(st2.s == st.s && st2.f == st.f);
        CHECK(st3.s == st.s && st3.f == st.f);
        st = t == WX_CHUNK / 16 ? st3 : (t & 1) ? st2 : st;
        CHECK(st.s < 0x10000u && st.f < 0x10000u);
        if (nown == 0) CHECK(st.s == 0xFFFFu && st.f == 0xFFFFu);
        sf[2 * (t >> 1)] |= st.s << (16 * (t & 1));
        sf[2 * (t >> 1) + 1] |= st.f << (16 * (t & 1));
    }
    for (int p = 0; p < WX_CHUNK && p < w.n; ++p) {
        const unsigned b0 = w.byte[p];
        // a word starts with an ASCII letter or digit, or with a non-ASCII char that is neither
        // whitespace nor isolated
        if (!(is_alnum(b0) || (b0 >= 0x80u && !w.na[p]))) continue;
        const Ref r = ref_setup(w, p);
        const int q = p + 1, k = q >> 5;
        const WxExtent e = wx_extent(wx_window(sf[2 * k], sf[2 * k + 2], q), wx_window(sf[2 * k + 1], sf[2 * k + 3], q), b0);
        CHECK(e.len == r.len);
        CHECK(e.fast == r.fast);
        if (b0 >= 0x80u) CHECK(e.len == 0 && !e.fast);
        const WxMask m = wx_keep_mask(e.len), l = wx_lower_keep(dword(w.byte + p), dword(w.byte + p + 4),
                                                                dword(w.byte + p + 8), dword(w.byte + p + 12), e.len);
        const uint32_t mm[4] = {m.x, m.y, m.z, m.w}, ll[4] = {l.x, l.y, l.z, l.w};
        for (int i = 0; i < 16; ++i) {
            CHECK(((mm[i >> 2] >> (8 * (i & 3))) & 0xFFu) == (i < r.len ? 0xFFu : 0u));
            CHECK(((ll[i >> 2] >> (8 * (i & 3))) & 0xFFu) == r.kept[i]);
        }
        ++checked;
    }
}

// expects (len, fast) at p besides the comparison with the earlier rule
static void expect(const Window &w, int p, int len, bool fast, const char *what) {
    check_window(w, what);
    const Ref r = ref_setup(w, p);
    CHECK(r.len == len);
    CHECK(r.fast == fast);
}

int main() {
    const char *what = "tables";
    // `| 0x20` is the lower-case form of every ASCII letter and digit, and of those only: among
    // the bytes it changes (the ones without the bit) it is right for A-Z and for nothing else
    for (unsigned b = 0; b < 256; ++b) {
        const bool same = (b | 0x20u) == lower(b);
        if (is_alnum(b)) CHECK(same);
        if (!is_alnum(b) && !(b & 0x20u)) CHECK(!same);
        const uint32_t x = b * 0x01010101u;
        CHECK(wx_gather4(wx_alnum4(x)) == (is_alnum(b) ? 0xFu : 0u));
        CHECK(wx_gather4(wx_term4(x)) == (b < 0x80u && (is_ws(b) || is_iso(b)) ? 0xFu : 0u));
        CHECK(wx_is_alnum(b) == is_alnum(b));
        CHECK(wx_is_term(b) == (b < 0x80u && (is_ws(b) || is_iso(b))));
    }
    for (uint32_t n4 = 0; n4 < 0x10000u; ++n4) {  // every four classes as nibbles
        if (n4 & 0xCCCCu) continue;
        uint32_t want = 0;
        for (int i = 0; i < 4; ++i) {
            const uint32_t c = (n4 >> (4 * i)) & 0xFu;
            want |= (uint32_t)(c == WX_V_WS || c == WX_V_ISO) << i | (uint32_t)(c == WX_V_OTHER) << (16 + i);
        }
        CHECK(wx_nibble_classes(n4) == want);
    }
    for (int n = 0; n <= 16; ++n) {
        const WxMask m = wx_keep_mask(n);
        const uint32_t mm[4] = {m.x, m.y, m.z, m.w};
        for (int i = 0; i < 16; ++i) CHECK(((mm[i >> 2] >> (8 * (i & 3))) & 0xFFu) == (i < n ? 0xFFu : 0u));
    }

    const std::string terms[] = {" ", ",", "\x01", "\x7F", "\xC3\xA9", "\xC2\xA0", "\xE2\x80\x94", "[MASK]"};
    // words of 15, 16, 17 and 33 bytes in front of every kind of end, at several alignments
    what = "word lengths";
    for (int len : {1, 2, 15, 16, 17, 33})
        for (int at : {0, 1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 500, 990})
            for (const std::string &t : terms) {
                Window w;
                for (int i = 0; i < SPAN; ++i) w.byte[i] = ' ';
                w.put(at, std::string((size_t)len, (char)('a' + len % 26)));
                w.byte[at] = 'Q';
                w.put(at + len, t);
                const bool na_t = (unsigned char)t[0] >= 0xC0u && t != "\xC3\xA9" && at + len < WX_CHUNK;
                if (na_t) w.na[at + len] = true;  // (e-acute is a letter: the rare pass leaves it)
                const bool term_fast = t == " " || t == "," || t == "[MASK]" || na_t;
                expect(w, at, len < 16 ? len : 16, len <= 16 && term_fast, what);
            }
    // a record start at p, p + 1, p + 15, p + 16 (and none) inside a long run of letters
    what = "record starts";
    for (int at : {0, 7, 16, 40, 1000, 1008, 1023})
        for (int d : {0, 1, 2, 15, 16, 17}) {
            Window w;
            for (int i = 0; i < SPAN; ++i) w.byte[i] = 'a' + i % 26;
            w.rec[at + d] = true;
            expect(w, at, d >= 1 && d <= 16 ? d : 16, d >= 1 && d <= 16, what);
        }
    // words that end at chunk offsets 1023, 1024, 1039 and 1040
    what = "chunk end";
    for (int end : {1023, 1024, 1039, 1040})
        for (int len : {1, 3, 15, 16, 17, 18})
            for (const std::string &t : terms) {
                const int at = end - len;
                if (at >= WX_CHUNK) continue;
                Window w;
                for (int i = 0; i < SPAN; ++i) w.byte[i] = '.';
                w.put(at, std::string((size_t)len, 'Z'));
                w.put(end, t);
                const bool lead = (unsigned char)t[0] >= 0xC0u && t != "\xC3\xA9";
                if (lead && end < WX_CHUNK) w.na[end] = true;  // the halo's chars are not looked up
                const bool term_fast = t == " " || t == "," || t == "[MASK]" || (lead && end < WX_CHUNK);
                expect(w, at, len < 16 ? len : 16, len <= 16 && term_fast, what);
                Window r = w;  // ... and a record start there instead
                r.rec[end] = true;
                expect(r, at, len < 16 ? len : 16, len <= 16, what);
            }
    // the text ends inside a word
    what = "text end";
    for (int at : {0, 5, 16, 1000, 1010, 1023})
        for (int d : {1, 2, 15, 16, 17}) {
            Window w;
            for (int i = 0; i < SPAN; ++i) w.byte[i] = 'a' + i % 26;
            w.cut(at + d);
            expect(w, at, d < 16 ? d : 16, d <= 16, what);
        }
    // a first byte at or above 0x80
    what = "non-ASCII first byte";
    for (int at : {0, 15, 16, 1023}) {
        Window w;
        for (int i = 0; i < SPAN; ++i) w.byte[i] = ' ';
        w.put(at, "\xC3\xA9tude ");
        expect(w, at, 0, false, what);
    }
    // all letters and digits; nothing at all (every lane empty); a chunk that ends in its first lane
    what = "all alphanumeric";
    {
        Window w;
        for (int i = 0; i < SPAN; ++i) w.byte[i] = "aZ09mQ"[i % 6];
        expect(w, 0, 16, false, what);
        expect(w, 1023, 16, false, what);
    }
    what = "empty lanes";
    {
        Window w;
        w.cut(0);
        check_window(w, what);
        Window v;
        for (int i = 0; i < SPAN; ++i) v.byte[i] = 'x';
        v.cut(5);
        expect(v, 0, 5, true, what);
        expect(v, 4, 1, true, what);
    }

    // random windows
    what = "random";
    std::mt19937 rng(9);
    const std::string letters = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ", digits = "0123456789",
                      punct = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~";
    for (int it = 0; it < 4000; ++it) {
        Window w;
        const int run = 1 + (int)(rng() % 24);  // mean run of letters
        for (int i = 0; i < SPAN; ++i) {
            unsigned b;
            if (rng() % (unsigned)(run + 1)) {
                b = rng() % 5 ? (unsigned char)letters[rng() % letters.size()] : (unsigned char)digits[rng() % 10];
            } else {
                switch (rng() % 10) {
                    case 0: case 1: case 2: b = " \t\n\r"[rng() % 4 ? 0 : rng() % 4]; break;
                    case 3: case 4: b = (unsigned char)punct[rng() % punct.size()]; break;
                    case 5: b = rng() % 32; break;
                    case 6: b = 0x7F; break;
                    case 7: b = 0x80 + rng() % 0x40; break;
                    case 8: b = 0xC0 + rng() % 0x40; break;
                    default: b = rng() % 256; break;
                }
            }
            w.byte[i] = (unsigned char)b;
            if (i < WX_CHUNK && b >= 0xC0u) w.na[i] = rng() % 2;
        }
        const int nrec = (int)(rng() % 12);
        for (int k = 0; k < nrec; ++k) w.rec[rng() % (SPAN + 1)] = true;
        if (rng() % 3 == 0) w.cut((int)(rng() % (SPAN + 1)));
        check_window(w, what);
    }
    if (fails || checked < 100000) {
        printf("wp_extent: %d failures, %ld piece starts checked\n", fails, checked);
        return 1;
    }
    printf("wp_extent ok (%ld piece starts)\n", checked);
    return 0;
}
