// Word extents of the WordPiece chunk kernel's first probes (tokenize_wordpiece.hip, step 4):
// two bitmaps over a chunk's bytes, built once per chunk from each lane's own 16 bytes, give a
// word's length and whether the fast path may take it in a handful of instructions per piece.
// Includes nothing from HIP, so a host program can call it (tests/test_wp_extent.py).
//
// Both bitmaps are indexed by chunk offset, 0 .. WX_BITS - 1: the chunk's bytes and the first 16
// of its right halo (a word of 16 bytes that starts at the chunk's last byte ends there).
//   S (stop): the byte is no ASCII letter or digit, or a record starts at it, or it lies at or
//     past the end of the text.  A word that starts at p runs to the first stop after p, capped
//     at 16 bytes.
//   F (fast terminator): the byte is ASCII whitespace or isolated punctuation, or the lead byte
//     of a non-ASCII whitespace/isolated char the rare pass found (inside the chunk only), or a
//     record starts at it, or it lies at or past the end of the text.  A word whose first byte is
//     ASCII and whose run of letters and digits ends at an F byte is the whole pre-token: one
//     probe of its lower-cased bytes decides it.  Any other end (a control byte, a non-ASCII
//     letter, a 17th letter) leaves the word to the general path.
// The words of the two bitmaps are interleaved (S word k, F word k, S word k + 1, ...), so the
// 64-bit windows of both at a piece come with one 16-byte read.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define WP_EXTENT_FN __host__ __device__ inline
#else
#define WP_EXTENT_FN inline
#endif

namespace sdl {

constexpr int WX_CHUNK = 1024;                 // = CHUNK
constexpr int WX_BITS = WX_CHUNK + 16;         // bits that are ever read
constexpr int WX_WORDS = WX_CHUNK / 32 + 2;    // words per bitmap: a window at bit 1024 reads words 32 and 33

constexpr uint32_t WX_B7 = 0x80808080u;

// 0x80 in every byte of x that is an ASCII letter or digit
WP_EXTENT_FN uint32_t wx_alnum4(uint32_t x) {
    const uint32_t hi = x & WX_B7;
    const uint32_t l = (x | 0x20202020u) & 0x7F7F7F7Fu;
    const uint32_t ge_a = (l + 0x1F1F1F1Fu) & WX_B7;   // l >= 0x61
    const uint32_t le_z = ~(l + 0x05050505u) & WX_B7;  // l <= 0x7A
    const uint32_t d = x & 0x7F7F7F7Fu;
    const uint32_t ge_0 = (d + 0x50505050u) & WX_B7;   // d >= 0x30
    const uint32_t le_9 = ~(d + 0x46464646u) & WX_B7;  // d <= 0x39
    return ((ge_a & le_z) | (ge_0 & le_9)) & ~hi;
}
// 0x80 in every byte of x that is ASCII whitespace (\t \n \r space) or ASCII isolated
// punctuation (printable, no letter or digit, not 0x7F)
WP_EXTENT_FN uint32_t wx_term4(uint32_t x) {
    const uint32_t a = x & 0x7F7F7F7Fu;
    const uint32_t ge9 = a + 0x77777777u, ge11 = a + 0x75757575u, ge13 = a + 0x73737373u, ge14 = a + 0x72727272u;
    const uint32_t ws = (ge9 & ~ge11) | (ge13 & ~ge14);          // 9, 10, 13 (bit 7 of each byte)
    const uint32_t pr = (a + 0x60606060u) & ~(a + 0x01010101u);  // 32 .. 126
    return (ws | pr) & ~x & ~wx_alnum4(x) & WX_B7;
}
// bit k = bit 7 of byte k
WP_EXTENT_FN uint32_t wx_gather4(uint32_t m) { return ((((m >> 7) & 0x01010101u) * 0x00204081u) >> 21) & 0xFu; }

// The same two masks from four bytes' visible classes as nibbles (byte k: bits 4k .. 4k + 3;
// letter or digit 3, whitespace 1, isolated 2, none 0 -- the ASCII classifier's values before
// any non-ASCII or added-token class is written over them): bits 0-3 whitespace or isolated,
// bits 16-19 letter or digit.  One multiply gathers both.
constexpr uint32_t WX_V_WS = 1, WX_V_ISO = 2, WX_V_OTHER = 3;
WP_EXTENT_FN uint32_t wx_nibble_classes(uint32_t n4) {
    const uint32_t one = (n4 ^ (n4 >> 1)) & 0x1111u, both = (n4 & (n4 >> 1)) & 0x1111u;
    const uint32_t g = (one | (both << 16)) * 0x1248u;  // bit 4k -> bit 12 + k, no two products meet
    return ((g >> 12) & 0xFu) | ((g >> 28) << 16);
}

// the same two classes of one byte
WP_EXTENT_FN bool wx_is_alnum(uint32_t b) { return (b | 0x20u) - 'a' < 26u || b - '0' < 10u; }
WP_EXTENT_FN bool wx_is_term(uint32_t b) { return (b - 32u < 95u && !wx_is_alnum(b)) || b - 9u < 2u || b == 13u; }

struct WxStops {
    uint32_t s, f;  // 16 bits each: bit i is byte i of the 16
};
// The S and F bits of 16 bytes.  an16, tm16: the bytes that are ASCII letters or digits, ASCII
// whitespace or isolated punctuation; rec16: a record starts at byte i; na16: byte i leads a
// non-ASCII whitespace/isolated char; nown: bytes i >= nown lie at or past the end of the text
// (0 .. 16).  wx_stops classifies the bytes b[0..3] (little-endian dwords) itself -- the plain
// form; the kernel takes an16 and tm16 from wx_nibble_classes (a lane's own bytes) and from
// ballots of wx_is_alnum / wx_is_term (the halo's), which the host check holds against it.
WP_EXTENT_FN WxStops wx_stops_from(uint32_t an16, uint32_t tm16, uint32_t rec16, uint32_t na16, int nown) {
    const uint32_t past = 0xFFFFu & ~((1u << nown) - 1u);
    const uint32_t hard = (rec16 & 0xFFFFu) | past;
    return WxStops{(~an16 & 0xFFFFu) | hard, (tm16 & 0xFFFFu) | (na16 & 0xFFFFu) | hard};
}
WP_EXTENT_FN WxStops wx_stops(const uint32_t b[4], uint32_t rec16, uint32_t na16, int nown) {
    uint32_t an = 0, tm = 0;
    for (int j = 0; j < 4; ++j) {
        an |= wx_gather4(wx_alnum4(b[j])) << (4 * j);
        tm |= wx_gather4(wx_term4(b[j])) << (4 * j);
    }
    return wx_stops_from(an, tm, rec16, na16, nown);
}

// 32 bits of a bitmap from bit `bit` on, out of the two words that hold them (lo: word bit >> 5).
WP_EXTENT_FN uint32_t wx_window(uint32_t lo, uint32_t hi, int bit) {
    return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (bit & 31));
}

struct WxExtent {
    int len;    // bytes of the word's leading run of ASCII letters and digits, 0 .. 16
    bool fast;  // the run is the whole pre-token
};
// A word at chunk offset p: sw, fw = wx_window of S and F at bit p + 1; first: the word's first
// byte.  (Bit 15 of the stop window is forced: the run is cut at 16 bytes, and F at p + 16 says
// whether the word ends there.)
WP_EXTENT_FN WxExtent wx_extent(uint32_t sw, uint32_t fw, uint32_t first) {
    const int run = __builtin_ctz(sw | 0x8000u);  // stop-free bytes after the first
    const bool ascii = (first & 0x80u) == 0u;
    return WxExtent{ascii ? run + 1 : 0, ascii && ((fw >> run) & 1u) != 0u};
}

struct WxMask {
    uint32_t x, y, z, w;
};
// 0xFF in the first n of 16 bytes (n in 0 .. 16): two 64-bit shifts, each in two halves so that
// no shift count reaches 64.
WP_EXTENT_FN WxMask wx_keep_mask(int n) {
    const int lo = n < 8 ? n : 8, hi = n - lo;
    const uint64_t a = ~((~0ull << (4 * lo)) << (4 * lo)), b = ~((~0ull << (4 * hi)) << (4 * hi));
    return WxMask{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
}
// Lower-case form of the first n bytes of a run of ASCII letters and digits, zero behind them:
// `| 0x20` turns A-Z into a-z and leaves a-z and 0-9 (which carry the bit) as they are.
WP_EXTENT_FN WxMask wx_lower_keep(uint32_t x, uint32_t y, uint32_t z, uint32_t w, int n) {
    const WxMask m = wx_keep_mask(n);
    return WxMask{(x | 0x20202020u) & m.x, (y | 0x20202020u) & m.y, (z | 0x20202020u) & m.z,
                  (w | 0x20202020u) & m.w};
}
// The first n bytes as they are, zero behind them: the word's form under a normalizer that
// keeps case.
WP_EXTENT_FN WxMask wx_keep(uint32_t x, uint32_t y, uint32_t z, uint32_t w, int n) {
    const WxMask m = wx_keep_mask(n);
    return WxMask{x & m.x, y & m.y, z & m.z, w & m.w};
}

}  // namespace sdl
