// zstd_format.hpp -- the Zstandard frame format (RFC 8878), for host and device.
//
// Everything that knows what the bytes of a .zst frame mean lives here and compiles both with a
// plain C++17 compiler (tests/zstd_host_model.cpp, sdl_zstd_split_frames) and as device code
// (zstd.hip): frame / block / literals-section / sequences-section headers, the Huffman weight
// decode and decode table, FSE tables from normalized counts, the predefined distributions, the
// code -> baseline / extra-bits tables, the repeat-offset rule (symbolic, so that a block can be
// decoded before its incoming history is known), and XXH64.  Every limit of the format is enforced
// here, not in the callers, and every read of compressed bytes goes through peek_bits(), which
// never touches a byte outside the section it was given.
//
// No dictionaries; offset codes above 31 and window logs above 31 are refused.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define ZS_HD __host__ __device__ inline
#else
#define ZS_HD inline
#endif

namespace zs {

// per-frame / per-block status (kernels.hpp names them ZS_E_*)
enum : int32_t {
    OK = 0,
    E_RANGE = 1,      // frame range outside the buffer, or out of order
    E_TRUNC = 2,      // input ends inside the frame
    E_MAGIC = 3,      // not a zstd frame, or a reserved bit set
    E_DICT = 4,       // Dictionary_ID present and non-zero
    E_WINDOW = 5,     // window log or offset code beyond the supported limit (31)
    E_BTYPE = 6,      // block type 3
    E_BSIZE = 7,      // block larger than Block_Maximum_Size
    E_LITHDR = 8,     // literals section header / stream sizes
    E_HUF = 9,        // Huffman tree description
    E_FSE = 10,       // FSE table description
    E_SEQHDR = 11,    // sequences section header, repeat of nothing, literal lengths over the literals
    E_ENDBITS = 12,   // a bitstream did not end exactly
    E_FAR = 13,       // match offset reaches before the frame's start (or is zero)
    E_SIZE = 14,      // decoded size != Frame_Content_Size
    E_CHECKSUM = 15,  // XXH64 content checksum mismatch
    E_STALL = 16      // a bounded loop ran out (a guard)
};

constexpr uint32_t MAGIC = 0xFD2FB528u;
constexpr uint32_t SKIP_MAGIC = 0x184D2A50u;  // .. 0x184D2A5F
constexpr uint32_t BLOCK_MAX = 128u << 10;
constexpr uint32_t HUF_MAX_BITS = 11;
constexpr uint32_t LL_MAX_LOG = 9, OF_MAX_LOG = 8, ML_MAX_LOG = 9, HW_MAX_LOG = 6;
constexpr uint32_t LL_MAX_SYM = 35, OF_MAX_SYM = 31, ML_MAX_SYM = 52;
constexpr uint32_t MAX_WINDOW_LOG = 31;

ZS_HD uint32_t hibit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }  // v != 0
ZS_HD uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
ZS_HD uint32_t le24(const uint8_t *p) { return le16(p) | (uint32_t)p[2] << 16; }
ZS_HD uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }
ZS_HD uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | (uint64_t)le32(p + 4) << 32; }

// ---- the one reader of compressed bits -------------------------------------------------------
// load64 is the only place that touches a section's bytes: the 8 bytes p[b0 .. b0 + 8) as a
// little-endian word, bytes outside [0, len) reading as zero -- no byte outside [p, p + len) is
// ever loaded, reading forward or backward.
ZS_HD uint64_t load64(const uint8_t *p, uint32_t len, int64_t b0) {
    if (b0 >= 0 && (uint64_t)b0 + 8 <= len) {
        uint64_t w;
        memcpy(&w, p + b0, 8);  // little-endian hosts and gfx9
        return w;
    }
    uint64_t w = 0;
    for (int i = 0; i < 8; ++i) {
        const int64_t k = b0 + i;
        if (k >= 0 && k < (int64_t)len) w |= (uint64_t)p[k] << (8 * i);
    }
    return w;
}

// Bits [bp, bp + n) of the section p[0 .. len), bit k being bit (k & 7) of byte k >> 3, n <= 32;
// bits outside the section read as zero.
ZS_HD uint32_t peek_bits(const uint8_t *p, uint32_t len, int64_t bp, uint32_t n) {
    if (n == 0) return 0;
    const int64_t b0 = bp >> 3;  // arithmetic: floor
    return (uint32_t)((load64(p, len, b0) >> (uint32_t)(bp - b0 * 8)) & ((1ull << n) - 1));
}

// A bitstream read backward from its end mark (Huffman streams, FSE streams).  pos = bits left;
// it goes negative when more was read than the stream holds (those bits read as zero).  The last
// word loaded is kept: w = bits [wbase, wbase + 64), refilled (through load64, the one place that
// touches the bytes) when a read leaves it.
struct BackBits {
    const uint8_t *p;
    uint32_t len;
    int64_t pos;
    uint64_t w;
    int64_t wbase;
    ZS_HD bool init(const uint8_t *s, uint32_t n) {
        p = s;
        len = n;
        pos = 0;
        w = 0;
        wbase = -(1ll << 40);  // (no word yet)
        if (n == 0 || s[n - 1] == 0) return false;
        pos = (int64_t)n * 8 - 8 + hibit(s[n - 1]);
        return true;
    }
    // bits [bp, bp + n), n <= 32
    ZS_HD uint32_t at(int64_t bp, uint32_t n) {
        if (n == 0) return 0;
        if (bp < wbase || bp + n > wbase + 64) {
            wbase = ((bp + n + 7) & ~7ll) - 64;  // the word ends at the first byte boundary at or past the read
            w = load64(p, len, wbase >> 3);
        }
        return (uint32_t)((w >> (uint32_t)(bp - wbase)) & ((1ull << n) - 1));
    }
    ZS_HD uint32_t read(uint32_t n) {
        pos -= n;
        return at(pos, n);
    }
    // the next n bits without consuming them, zero-filled below the stream's first bit
    ZS_HD uint32_t peek(uint32_t n) { return at(pos - (int64_t)n, n); }
};

// ---- frame and block headers -----------------------------------------------------------------
struct FrameInfo {
    uint32_t skippable;    // 1: a skippable frame (hdr = 8, content = its size field)
    uint32_t hdr;          // header bytes, magic included
    uint32_t has_fcs, checksum;
    uint32_t block_max;    // min(window, 128 KiB)
    uint64_t fcs;          // Frame_Content_Size, when has_fcs
    uint64_t window;
    uint64_t skip_size;
};

ZS_HD int32_t frame_header(const uint8_t *p, uint64_t avail, FrameInfo &f) {
    f = FrameInfo{};
    if (avail < 4) return E_TRUNC;
    const uint32_t magic = le32(p);
    if ((magic & 0xFFFFFFF0u) == SKIP_MAGIC) {
        if (avail < 8) return E_TRUNC;
        f.skippable = 1;
        f.hdr = 8;
        f.skip_size = le32(p + 4);
        return OK;
    }
    if (magic != MAGIC) return E_MAGIC;
    if (avail < 5) return E_TRUNC;
    const uint32_t fhd = p[4];
    const uint32_t fcs_flag = fhd >> 6, single = (fhd >> 5) & 1, did_flag = fhd & 3;
    if (fhd & 0x08) return E_MAGIC;  // reserved bit
    const uint32_t did_bytes = did_flag == 3 ? 4 : did_flag;
    const uint32_t fcs_bytes = fcs_flag == 0 ? single : (1u << fcs_flag);
    const uint32_t hdr = 5 + (single ? 0 : 1) + did_bytes + fcs_bytes;
    if (avail < hdr) return E_TRUNC;
    uint32_t q = 5;
    uint64_t window = 0;
    if (!single) {
        const uint32_t wd = p[q++];
        const uint32_t wlog = 10 + (wd >> 3);
        if (wlog > MAX_WINDOW_LOG) return E_WINDOW;
        window = (1ull << wlog) + ((1ull << wlog) >> 3) * (wd & 7);
    }
    uint32_t did = 0;
    for (uint32_t i = 0; i < did_bytes; ++i) did |= (uint32_t)p[q++] << (8 * i);
    uint64_t fcs = 0;
    for (uint32_t i = 0; i < fcs_bytes; ++i) fcs |= (uint64_t)p[q++] << (8 * i);
    if (fcs_bytes == 2) fcs += 256;
    f.hdr = hdr;
    f.has_fcs = fcs_bytes != 0;
    f.fcs = fcs;
    f.checksum = (fhd >> 2) & 1;
    if (single) window = fcs;
    f.window = window;
    f.block_max = window < BLOCK_MAX ? (uint32_t)window : BLOCK_MAX;
    return did != 0 ? E_DICT : OK;  // (the header is complete either way: the frame's extent can be walked)
}

struct BlockHdr {
    uint32_t last, type, size;  // size: Block_Size (RLE: the regenerated size)
    uint32_t content;           // bytes of content after the 3-byte header (RLE: 1)
};

// the block header at p (avail bytes to the end of the range)
ZS_HD int32_t block_header(const uint8_t *p, uint64_t avail, uint32_t block_max, BlockHdr &b) {
    if (avail < 3) return E_TRUNC;
    const uint32_t h = le24(p);
    b.last = h & 1;
    b.type = (h >> 1) & 3;
    b.size = h >> 3;
    if (b.type == 3) return E_BTYPE;
    if (b.size > block_max) return E_BSIZE;
    b.content = b.type == 1 ? 1 : b.size;
    if (avail < 3 + (uint64_t)b.content) return E_TRUNC;
    return OK;
}

// Walks one frame's headers (no entropy decode): its length in bytes and its block count.
ZS_HD int32_t frame_extent(const uint8_t *p, uint64_t avail, FrameInfo &f, uint64_t &bytes, uint32_t &n_blocks) {
    bytes = 0;
    n_blocks = 0;
    int32_t st = frame_header(p, avail, f);
    if (st && st != E_DICT) return st;  // a frame that names a dictionary is a frame; decoding refuses it
    if (f.skippable) {
        if (avail < 8 + f.skip_size) return E_TRUNC;
        bytes = 8 + f.skip_size;
        return OK;
    }
    uint64_t q = f.hdr;
    for (uint64_t guard = avail / 3 + 2; guard; --guard) {
        BlockHdr b;
        st = block_header(p + q, avail - q, f.block_max, b);
        if (st) return st;
        q += 3 + b.content;
        ++n_blocks;
        if (b.last) {
            if (f.checksum) {
                if (avail < q + 4) return E_TRUNC;
                q += 4;
            }
            bytes = q;
            return OK;
        }
    }
    return E_STALL;
}

// ---- FSE --------------------------------------------------------------------------------------
struct FseEntry {
    uint16_t base;
    uint8_t sym, nbits;
};

// Reads an FSE table description (normalized counts) from p[0 .. len).  norm may be null (the
// description is only measured).  Sets the accuracy log, the symbol count and the bytes used.
ZS_HD int32_t read_ncount(const uint8_t *p, uint32_t len, uint32_t max_log, uint32_t max_sym, int16_t *norm,
                          uint32_t &log, uint32_t &nsym, uint32_t &used) {
    int64_t bp = 0;
    log = 5 + peek_bits(p, len, bp, 4);
    bp += 4;
    if (log > max_log) return E_FSE;
    int32_t remaining = 1 << log;
    uint32_t s = 0;
    while (remaining > 0 && s <= max_sym) {
        const uint32_t bits = hibit((uint32_t)remaining + 1) + 1;
        uint32_t val = peek_bits(p, len, bp, bits);
        bp += bits;
        const uint32_t lower = (1u << (bits - 1)) - 1;
        const uint32_t threshold = (1u << bits) - 1 - ((uint32_t)remaining + 1);
        if ((val & lower) < threshold) {
            bp -= 1;
            val &= lower;
        } else if (val > lower) {
            val -= threshold;
        }
        const int32_t proba = (int32_t)val - 1;
        remaining -= proba < 0 ? -proba : proba;
        if (norm) norm[s] = (int16_t)proba;
        ++s;
        if (proba == 0) {
            for (uint32_t guard = 0; guard < 128; ++guard) {
                const uint32_t rep = peek_bits(p, len, bp, 2);
                bp += 2;
                for (uint32_t i = 0; i < rep; ++i) {
                    if (s > max_sym) return E_FSE;
                    if (norm) norm[s] = 0;
                    ++s;
                }
                if (rep != 3) break;
            }
        }
        if ((uint64_t)bp > (uint64_t)len * 8 + 64) return E_TRUNC;
    }
    if (remaining != 0 || s > max_sym + 1) return E_FSE;
    used = (uint32_t)((bp + 7) >> 3);
    if (used > len) return E_TRUNC;
    nsym = s;
    return OK;
}

// The decode table of 1 << log entries from normalized counts ("less than 1" = -1).  cnt is
// scratch for nsym 16-bit words.
ZS_HD int32_t fse_build(const int16_t *norm, uint32_t nsym, uint32_t log, FseEntry *tab, uint16_t *cnt) {
    const uint32_t size = 1u << log, mask = size - 1;
    uint32_t high = size;
    for (uint32_t s = 0; s < nsym; ++s) {
        if (norm[s] == -1) {
            if (high == 0) return E_FSE;
            tab[--high].sym = (uint8_t)s;
            cnt[s] = 1;
        }
    }
    const uint32_t step = (size >> 1) + (size >> 3) + 3;
    uint32_t pos = 0, placed = size - high;
    for (uint32_t s = 0; s < nsym; ++s) {
        if (norm[s] <= 0) continue;
        cnt[s] = (uint16_t)norm[s];
        placed += (uint32_t)norm[s];
        if (placed > size) return E_FSE;
        for (int32_t i = 0; i < norm[s]; ++i) {
            tab[pos].sym = (uint8_t)s;
            do {
                pos = (pos + step) & mask;
            } while (pos >= high);
        }
    }
    if (pos != 0 || placed != size) return E_FSE;
    for (uint32_t i = 0; i < size; ++i) {
        const uint32_t d = cnt[tab[i].sym]++;
        const uint32_t nb = log - hibit(d);
        tab[i].nbits = (uint8_t)nb;
        tab[i].base = (uint16_t)((d << nb) - size);
    }
    return OK;
}

// ---- predefined distributions and code tables -------------------------------------------------
ZS_HD int16_t predef_norm(uint32_t which, uint32_t i) {  // which: 0 LL, 1 OF, 2 ML
    constexpr int8_t LL[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                               2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    constexpr int8_t OF[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    constexpr int8_t ML[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                               1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    return which == 0 ? LL[i] : which == 1 ? OF[i] : ML[i];
}
ZS_HD uint32_t predef_nsym(uint32_t which) { return which == 0 ? 36 : which == 1 ? 29 : 53; }
ZS_HD uint32_t predef_log(uint32_t which) { return which == 1 ? 5 : 6; }

ZS_HD uint32_t ll_base(uint32_t c) {
    constexpr uint32_t T[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,   9,   10,  11,   12,   13,   14,   15,    16,    18,
                                20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
    return T[c];
}
ZS_HD uint32_t ll_bits(uint32_t c) {
    constexpr uint8_t T[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1,
                               1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    return T[c];
}
ZS_HD uint32_t ml_base(uint32_t c) {
    constexpr uint32_t T[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13,  14,  15,  16,   17,   18,   19,   20,
                                21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31,  32,  33,  34,   35,   37,   39,   41,
                                43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
    return T[c];
}
ZS_HD uint32_t ml_bits(uint32_t c) {
    constexpr uint8_t T[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                               0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    return T[c];
}

// ---- Huffman ----------------------------------------------------------------------------------
struct HufEntry {
    uint8_t sym, nbits;
};

// scratch for the table builders (LDS on the device)
struct Work {
    int16_t norm[256];
    uint16_t cnt[256];
    uint8_t weights[256];
    FseEntry wtab[1 << HW_MAX_LOG];
    uint32_t rank[HUF_MAX_BITS + 2];
};

// Bytes of the Huffman tree description at d (avail >= 1 bytes), from its first byte alone.
ZS_HD uint32_t huf_desc_bytes(uint32_t hb) { return hb < 128 ? 1 + hb : 1 + (hb - 127 + 1) / 2; }

// FSE-compressed Huffman weights: p[0 .. len) -> weights[0 .. n), n <= 255.
ZS_HD int32_t huf_fse_weights(const uint8_t *p, uint32_t len, Work &w, uint32_t &n) {
    uint32_t log, nsym, used;
    int32_t st = read_ncount(p, len, HW_MAX_LOG, 255, w.norm, log, nsym, used);
    if (st) return st == E_FSE || st == E_TRUNC ? E_HUF : st;
    if (fse_build(w.norm, nsym, log, w.wtab, w.cnt)) return E_HUF;
    BackBits r;
    if (!r.init(p + used, len - used)) return E_HUF;
    uint32_t s1 = r.read(log), s2 = r.read(log);
    if (r.pos < 0) return E_HUF;
    n = 0;
    for (;;) {
        if (n > 253) return E_HUF;
        w.weights[n++] = w.wtab[s1].sym;
        s1 = w.wtab[s1].base + r.read(w.wtab[s1].nbits);
        if (r.pos < 0) {
            w.weights[n++] = w.wtab[s2].sym;
            break;
        }
        if (n > 253) return E_HUF;
        w.weights[n++] = w.wtab[s2].sym;
        s2 = w.wtab[s2].base + r.read(w.wtab[s2].nbits);
        if (r.pos < 0) {
            w.weights[n++] = w.wtab[s1].sym;
            break;
        }
    }
    return OK;
}

// The Huffman decode table (1 << log entries, log <= 11, tab holds 2048) from the tree
// description at d[0 .. avail).
ZS_HD int32_t huf_build(const uint8_t *d, uint32_t avail, HufEntry *tab, uint32_t &log, Work &w) {
    if (avail < 1) return E_HUF;
    const uint32_t hb = d[0];
    if (huf_desc_bytes(hb) > avail) return E_HUF;
    uint32_t n;
    if (hb >= 128) {
        n = hb - 127;
        for (uint32_t i = 0; i < n; ++i) w.weights[i] = (i & 1) ? (d[1 + i / 2] & 15) : (d[1 + i / 2] >> 4);
    } else {
        const int32_t st = huf_fse_weights(d + 1, hb, w, n);
        if (st) return st;
    }
    uint32_t sum = 0;
    for (uint32_t i = 0; i <= HUF_MAX_BITS + 1; ++i) w.rank[i] = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t x = w.weights[i];
        if (x > HUF_MAX_BITS) return E_HUF;
        if (x) sum += 1u << (x - 1);
        w.rank[x]++;
    }
    if (sum == 0) return E_HUF;
    log = hibit(sum) + 1;
    if (log > HUF_MAX_BITS) return E_HUF;
    const uint32_t left = (1u << log) - sum;
    if (left & (left - 1)) return E_HUF;  // the implied last weight must be a power of two
    const uint32_t last = hibit(left) + 1;
    w.weights[n++] = (uint8_t)last;
    w.rank[last]++;
    if (w.rank[1] < 2 || (w.rank[1] & 1)) return E_HUF;
    uint32_t start = 0;
    for (uint32_t x = 1; x <= log; ++x) {  // rank[x] becomes the first table index of weight x
        const uint32_t c = w.rank[x];
        w.rank[x] = start;
        start += c << (x - 1);
    }
    if (start != (1u << log)) return E_HUF;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t x = w.weights[s];
        if (!x) continue;
        const uint32_t cnt = 1u << (x - 1);
        uint32_t at = w.rank[x];
        w.rank[x] += cnt;
        if (at + cnt > (1u << log)) return E_HUF;
        for (uint32_t j = 0; j < cnt; ++j) tab[at + j] = HufEntry{(uint8_t)s, (uint8_t)(log + 1 - x)};
    }
    return OK;
}

// One Huffman stream src[0 .. len) -> exactly n bytes at dst (the caller owns dst[0 .. n)).
ZS_HD int32_t huf_stream(const HufEntry *tab, uint32_t log, const uint8_t *src, uint32_t len, uint8_t *dst, uint32_t n) {
    BackBits r;
    if (!r.init(src, len)) return E_ENDBITS;
    for (uint32_t i = 0; i < n; ++i) {
        const HufEntry e = tab[r.peek(log)];
        r.pos -= e.nbits;
        dst[i] = e.sym;
        if (r.pos < 0) return E_ENDBITS;
    }
    return r.pos == 0 ? OK : E_ENDBITS;
}

// ---- literals and sequences section headers ---------------------------------------------------
struct Sections {
    uint32_t lit_type;      // 0 raw, 1 RLE, 2 compressed, 3 treeless
    uint32_t n_streams;     // 1 or 4 (types 2, 3)
    uint32_t regen;         // regenerated literals
    uint32_t lit_hdr;       // literals header bytes
    uint32_t huf_desc;      // offset of the tree description (type 2)
    uint32_t huf_desc_len;
    uint32_t streams;       // offset and bytes of the stream area (jump table included) / raw bytes / RLE byte
    uint32_t streams_len;
    uint32_t nseq;
    uint32_t nseq_bytes;    // 1, 2 or 3
    uint32_t mode[3];       // LL, OF, ML: 0 predefined, 1 RLE, 2 FSE, 3 repeat
    uint32_t tab[3];        // offset of each table's description (mode 2) or byte (mode 1)
    uint32_t tab_len[3];
    uint32_t bits, bits_len;  // the sequence bitstream
};

ZS_HD uint32_t table_max_log(uint32_t t) { return t == 0 ? LL_MAX_LOG : t == 1 ? OF_MAX_LOG : ML_MAX_LOG; }
ZS_HD uint32_t table_max_sym(uint32_t t) { return t == 0 ? LL_MAX_SYM : t == 1 ? OF_MAX_SYM : ML_MAX_SYM; }

// The two section headers of a compressed block b[0 .. n); offsets are from b.
ZS_HD int32_t parse_sections(const uint8_t *b, uint32_t n, uint32_t block_max, Sections &s) {
    s = Sections{};
    if (n < 1) return E_LITHDR;
    const uint32_t b0 = b[0];
    const uint32_t type = b0 & 3, sf = (b0 >> 2) & 3;
    s.lit_type = type;
    uint32_t content;
    if (type < 2) {
        if (!(sf & 1)) {
            s.lit_hdr = 1;
            s.regen = b0 >> 3;
        } else if (sf == 1) {
            if (n < 2) return E_LITHDR;
            s.lit_hdr = 2;
            s.regen = le16(b) >> 4;
        } else {
            if (n < 3) return E_LITHDR;
            s.lit_hdr = 3;
            s.regen = le24(b) >> 4;
        }
        content = type == 0 ? s.regen : 1;
        s.streams = s.lit_hdr;
        s.streams_len = content;
    } else {
        uint32_t comp;
        if (sf < 2) {
            if (n < 3) return E_LITHDR;
            const uint32_t v = le24(b) >> 4;
            s.lit_hdr = 3;
            s.regen = v & 0x3FF;
            comp = v >> 10;
        } else if (sf == 2) {
            if (n < 4) return E_LITHDR;
            const uint32_t v = le32(b) >> 4;
            s.lit_hdr = 4;
            s.regen = v & 0x3FFF;
            comp = v >> 14;
        } else {
            if (n < 5) return E_LITHDR;
            const uint64_t v = ((uint64_t)le32(b) | (uint64_t)b[4] << 32) >> 4;
            s.lit_hdr = 5;
            s.regen = (uint32_t)(v & 0x3FFFF);
            comp = (uint32_t)(v >> 18);
        }
        s.n_streams = sf == 0 ? 1 : 4;
        content = comp;
        if ((uint64_t)s.lit_hdr + comp > n) return E_LITHDR;
        uint32_t desc = 0;
        if (type == 2) {
            if (comp < 1) return E_LITHDR;
            desc = huf_desc_bytes(b[s.lit_hdr]);
            if (desc > comp) return E_HUF;
            s.huf_desc = s.lit_hdr;
            s.huf_desc_len = desc;
        }
        s.streams = s.lit_hdr + desc;
        s.streams_len = comp - desc;
        if (s.regen == 0 || s.streams_len < (s.n_streams == 4 ? 10u : 1u)) return E_LITHDR;
    }
    if (s.regen > block_max) return E_LITHDR;
    if ((uint64_t)s.lit_hdr + content > n) return E_LITHDR;
    // sequences section
    uint32_t q = s.lit_hdr + content;
    if (q >= n) return E_SEQHDR;
    const uint32_t n0 = b[q];
    if (n0 == 0) {
        s.nseq_bytes = 1;
        if (q + 1 != n) return E_SEQHDR;
        return OK;
    }
    if (n0 < 128) {
        s.nseq = n0;
        s.nseq_bytes = 1;
    } else if (n0 < 255) {
        if (q + 2 > n) return E_SEQHDR;
        s.nseq = ((n0 - 128) << 8) + b[q + 1];
        s.nseq_bytes = 2;
    } else {
        if (q + 3 > n) return E_SEQHDR;
        s.nseq = le16(b + q + 1) + 0x7F00;
        s.nseq_bytes = 3;
    }
    q += s.nseq_bytes;
    if (s.nseq > block_max / 3) return E_SEQHDR;  // every match is >= 3 bytes of the block's output
    if (q >= n) return E_SEQHDR;
    const uint32_t modes = b[q++];
    if (modes & 3) return E_SEQHDR;  // reserved bits
    s.mode[0] = modes >> 6;
    s.mode[1] = (modes >> 4) & 3;
    s.mode[2] = (modes >> 2) & 3;
    for (uint32_t t = 0; t < 3; ++t) {
        s.tab[t] = q;
        if (s.mode[t] == 1) {
            if (q >= n) return E_SEQHDR;
            if (b[q] > table_max_sym(t)) return t == 1 ? E_WINDOW : E_FSE;
            s.tab_len[t] = 1;
        } else if (s.mode[t] == 2) {
            uint32_t log, nsym, used;
            // an offset-code table may name codes up to 255 in the format; codes above 31 are refused
            const int32_t st = read_ncount(b + q, n - q, table_max_log(t), table_max_sym(t), nullptr, log, nsym, used);
            if (st) return st == E_TRUNC ? E_FSE : st;
            s.tab_len[t] = used;
        }
        q += s.tab_len[t];
    }
    if (q >= n) return E_SEQHDR;
    s.bits = q;
    s.bits_len = n - q;
    return OK;
}

// The four (or one) Huffman streams of a literals section: area[0 .. total) is the jump table and
// the streams; stream k is area[off[k] .. off[k] + len[k]) and regenerates dlen[k] bytes at doff[k].
ZS_HD int32_t huf_split(const uint8_t *area, uint32_t total, uint32_t n_streams, uint32_t regen, uint32_t off[4],
                        uint32_t len[4], uint32_t doff[4], uint32_t dlen[4]) {
    if (n_streams == 1) {
        off[0] = 0;
        len[0] = total;
        doff[0] = 0;
        dlen[0] = regen;
        for (int k = 1; k < 4; ++k) off[k] = len[k] = doff[k] = dlen[k] = 0;
        return total ? OK : E_LITHDR;
    }
    if (total < 10) return E_LITHDR;
    const uint32_t l1 = le16(area), l2 = le16(area + 2), l3 = le16(area + 4);
    if (6ull + l1 + l2 + l3 >= total) return E_LITHDR;
    const uint32_t seg = (regen + 3) / 4;
    if (3 * seg > regen) return E_LITHDR;
    len[0] = l1, len[1] = l2, len[2] = l3, len[3] = total - 6 - l1 - l2 - l3;
    off[0] = 6, off[1] = 6 + l1, off[2] = 6 + l1 + l2, off[3] = 6 + l1 + l2 + l3;
    for (uint32_t k = 0; k < 4; ++k) doff[k] = k * seg, dlen[k] = k < 3 ? seg : regen - 3 * seg;
    return OK;
}

// One sequence table (t: 0 LL, 1 OF, 2 ML) from its defining block: mode 0 predefined, 1 the RLE
// byte at d, 2 the description at d[0 .. avail).  tab holds 1 << table_max_log(t) entries.
ZS_HD int32_t seq_table(uint32_t t, uint32_t mode, const uint8_t *d, uint32_t avail, FseEntry *tab, uint32_t &log, Work &w) {
    if (mode == 1) {
        if (avail < 1 || d[0] > table_max_sym(t)) return t == 1 ? E_WINDOW : E_FSE;
        tab[0] = FseEntry{0, d[0], 0};
        log = 0;
        return OK;
    }
    uint32_t nsym;
    if (mode == 0) {
        nsym = predef_nsym(t);
        log = predef_log(t);
        for (uint32_t i = 0; i < nsym; ++i) w.norm[i] = predef_norm(t, i);
    } else if (mode == 2) {
        uint32_t used;
        const int32_t st = read_ncount(d, avail, table_max_log(t), table_max_sym(t), w.norm, log, nsym, used);
        if (st) return st == E_TRUNC ? E_FSE : st;
    } else {
        return E_SEQHDR;
    }
    return fse_build(w.norm, nsym, log, tab, w.cnt);
}

// ---- repeat offsets, symbolically -------------------------------------------------------------
// A block is decoded before the history entering it is known, so each of the three slots, and
// each sequence's offset, is either a constant (kind 0, val = the offset) or "incoming slot
// kind - 1, minus val".
struct RepSlot {
    uint32_t kind, val;
};
struct RepMap {
    RepSlot s[3];
};
ZS_HD RepMap rep_identity() { return RepMap{{{1, 0}, {2, 0}, {3, 0}}}; }

// the value of a slot given the history `in` entering the block; 0 = invalid (before the start)
ZS_HD uint32_t rep_resolve(RepSlot r, const uint32_t in[3]) {
    if (r.kind == 0) return r.val;
    const uint32_t x = in[r.kind - 1];
    return x > r.val ? x - r.val : 0;
}

ZS_HD RepSlot rep_minus1(RepSlot r) {
    if (r.kind == 0) return RepSlot{0, r.val ? r.val - 1 : 0};
    return RepSlot{r.kind, r.val + 1};
}

// The offset of a sequence with Offset_Value ov, and the history update.
ZS_HD RepSlot rep_apply(RepMap &m, uint32_t ov, bool ll0) {
    RepSlot o;
    if (ov > 3) {
        o = RepSlot{0, ov - 3};
    } else {
        const uint32_t idx = ov - 1 + (ll0 ? 1 : 0);
        if (idx == 0) return m.s[0];
        o = idx == 3 ? rep_minus1(m.s[0]) : m.s[idx];
        if (idx == 1) {
            m.s[1] = m.s[0];
            m.s[0] = o;
            return o;
        }
    }
    m.s[2] = m.s[1];
    m.s[1] = m.s[0];
    m.s[0] = o;
    return o;
}

// One decoded sequence, positions relative to its block: its literals are
// lit[lit_end - ll .. lit_end) with ll = lit_end - (the previous record's lit_end), copied to
// [dst - ll, dst); the match is ml bytes at dst.  ml_kind = ml | kind << 30, off as RepSlot.val.
struct SeqRec {
    uint32_t lit_end, dst, ml_kind, off;
};
constexpr uint32_t ML_MASK = (1u << 30) - 1;

// Decodes the nseq sequences of one block into rec[0 .. nseq) (the caller owns that extent).
// stats (may be null): [ (ov - 1) * 2 + (ll == 0) ] counts of Offset_Value 1, 2, 3.
ZS_HD int32_t decode_sequences(const uint8_t *bits, uint32_t bits_len, uint32_t nseq, const FseEntry *llt, uint32_t ll_log,
                               const FseEntry *oft, uint32_t of_log, const FseEntry *mlt, uint32_t ml_log, uint32_t regen,
                               uint32_t block_max, SeqRec *rec, RepMap &map, uint32_t &out_size, uint32_t *stats) {
    BackBits r;
    if (!r.init(bits, bits_len)) return E_ENDBITS;
    uint32_t sl = r.read(ll_log), so = r.read(of_log), sm = r.read(ml_log);
    if (r.pos < 0) return E_ENDBITS;
    uint32_t lit_end = 0, out = 0;
    for (uint32_t i = 0; i < nseq; ++i) {
        const uint32_t lc = llt[sl].sym, oc = oft[so].sym, mc = mlt[sm].sym;
        if (lc > LL_MAX_SYM || mc > ML_MAX_SYM) return E_FSE;
        if (oc > OF_MAX_SYM) return E_WINDOW;
        const uint32_t ov = (1u << oc) + r.read(oc);
        const uint32_t ml = ml_base(mc) + r.read(ml_bits(mc));
        const uint32_t ll = ll_base(lc) + r.read(ll_bits(lc));
        if (i + 1 < nseq) {
            sl = llt[sl].base + r.read(llt[sl].nbits);
            sm = mlt[sm].base + r.read(mlt[sm].nbits);
            so = oft[so].base + r.read(oft[so].nbits);
        }
        if (r.pos < 0) return E_ENDBITS;
        lit_end += ll;
        if (lit_end > regen) return E_SEQHDR;
        const uint32_t dst = out + ll;
        out = dst + ml;
        if (out > block_max) return E_BSIZE;
        if (stats && ov <= 3) stats[(ov - 1) * 2 + (ll == 0)]++;
        const RepSlot o = rep_apply(map, ov, ll == 0);
        rec[i] = SeqRec{lit_end, dst, ml | o.kind << 30, o.val};
    }
    if (r.pos != 0) return E_ENDBITS;
    out_size = out + (regen - lit_end);
    if (out_size > block_max) return E_BSIZE;
    return OK;
}

// ---- XXH64 ------------------------------------------------------------------------------------
constexpr uint64_t XP1 = 0x9E3779B185EBCA87ull, XP2 = 0xC2B2AE3D27D4EB4Full, XP3 = 0x165667B19E3779F9ull,
                   XP4 = 0x85EBCA77C2B2AE63ull, XP5 = 0x27D4EB2F165667C5ull;
ZS_HD uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
ZS_HD uint64_t xxh_round(uint64_t acc, uint64_t in) { return rotl64(acc + in * XP2, 31) * XP1; }
ZS_HD uint64_t xxh_lane_seed(uint32_t lane) {  // seed 0
    return lane == 0 ? XP1 + XP2 : lane == 1 ? XP2 : lane == 2 ? 0 : 0 - XP1;
}
ZS_HD uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0, v)) * XP1 + XP4; }
// the hash from the four lane accumulators (used when len >= 32) and the tail p[0 .. len & 31)
ZS_HD uint64_t xxh_finish(const uint64_t v[4], const uint8_t *tail, uint64_t len) {
    uint64_t h;
    if (len >= 32) {
        h = rotl64(v[0], 1) + rotl64(v[1], 7) + rotl64(v[2], 12) + rotl64(v[3], 18);
        for (int i = 0; i < 4; ++i) h = xxh_merge(h, v[i]);
    } else {
        h = XP5;
    }
    h += len;
    uint32_t n = (uint32_t)(len & 31);
    for (; n >= 8; n -= 8, tail += 8) h = rotl64(h ^ xxh_round(0, le64(tail)), 27) * XP1 + XP4;
    if (n >= 4) {
        h = rotl64(h ^ (uint64_t)le32(tail) * XP1, 23) * XP2 + XP3;
        tail += 4;
        n -= 4;
    }
    for (; n; --n, ++tail) h = rotl64(h ^ (uint64_t)*tail * XP5, 11) * XP1;
    h ^= h >> 33;
    h *= XP2;
    h ^= h >> 29;
    h *= XP3;
    h ^= h >> 32;
    return h;
}
ZS_HD uint64_t xxh64(const uint8_t *p, uint64_t len) {
    uint64_t v[4];
    for (uint32_t i = 0; i < 4; ++i) v[i] = xxh_lane_seed(i);
    const uint64_t stripes = len / 32;
    for (uint64_t s = 0; s < stripes; ++s)
        for (uint32_t i = 0; i < 4; ++i) v[i] = xxh_round(v[i], le64(p + s * 32 + i * 8));
    return xxh_finish(v, p + stripes * 32, len);
}

// ---- one block's records, as the stages pass them on ------------------------------------------
// (zstd.hip keeps an array of these in device memory; the host model the same array on the host)
struct Block {
    uint32_t frame;        // stage 1
    uint32_t src;          // offset of the block's content in the input
    uint32_t size;         // content bytes (RLE: 1)
    uint32_t type, last;
    uint32_t rsize;        // regenerated size of a raw / RLE block
    Sections sec;          // stage 2 (compressed blocks)
    uint32_t huf_def;      // stage 3: the block whose tree / tables this one uses (itself, or earlier)
    uint32_t tab_def[3];
    uint32_t lit_base;     // literal arena, sequence arena
    uint32_t seq_base;
    RepMap map;            // stage 4
    uint32_t out_size;
    uint32_t rep_in[3];    // stage 5
    uint32_t out_base;     // in the call's output
    int32_t status;
};
constexpr uint32_t NO_BLOCK = 0xFFFFFFFFu;

struct Frame {
    uint32_t src, end;     // byte range in the input
    uint32_t first_block, n_blocks;
    uint32_t skippable, has_fcs, checksum, block_max;
    uint64_t fcs;
    uint32_t sum_off;      // offset of the 4 checksum bytes
    uint32_t out_base, out_size;
    uint32_t lit_total, seq_total;  // (scratch for the scans)
    int32_t status;
};

// ---- the serial parts of the stages, shared by zstd.hip and the host model ---------------------
// Stage 1, one frame: fills F and (when blocks != null) its block records from first_block on.
ZS_HD int32_t index_frame(const uint8_t *zst, uint64_t a, uint64_t z, uint32_t f, Frame &F, Block *blocks, uint32_t block_cap) {
    FrameInfo fi;
    F.src = (uint32_t)a;
    F.end = (uint32_t)z;
    F.n_blocks = 0;
    F.out_base = F.out_size = F.lit_total = F.seq_total = 0;
    int32_t st = frame_header(zst + a, z - a, fi);
    F.skippable = fi.skippable;
    F.has_fcs = fi.has_fcs;
    F.checksum = fi.checksum;
    F.block_max = fi.block_max;
    F.fcs = fi.fcs;
    F.sum_off = 0;
    if (st) return F.status = st;
    if (fi.skippable) return F.status = (z - a == 8 + fi.skip_size) ? OK : (z - a < 8 + fi.skip_size ? E_TRUNC : E_RANGE);
    uint64_t q = a + fi.hdr;
    uint32_t n = 0;
    for (uint64_t guard = (z - a) / 3 + 2; guard; --guard) {
        BlockHdr h;
        st = block_header(zst + q, z - q, fi.block_max, h);
        if (st) break;
        if (blocks) {
            if (F.first_block + n >= block_cap) {
                st = E_STALL;
                break;
            }
            Block &B = blocks[F.first_block + n];
            B.frame = f;
            B.src = (uint32_t)(q + 3);
            B.size = h.content;
            B.type = h.type;
            B.last = h.last;
            B.rsize = h.type == 2 ? 0 : h.size;
            B.huf_def = B.tab_def[0] = B.tab_def[1] = B.tab_def[2] = NO_BLOCK;
            B.lit_base = B.seq_base = B.out_size = B.out_base = 0;
            B.map = rep_identity();
            B.status = OK;
            B.sec = Sections{};
        }
        ++n;
        q += 3 + h.content;
        if (h.last) {
            if (fi.checksum) {
                if (z < q + 4) {
                    st = E_TRUNC;
                    break;
                }
                F.sum_off = (uint32_t)q;
                q += 4;
            }
            if (q != z) st = E_RANGE;  // the range must be exactly one frame
            break;
        }
        if (guard == 1) st = E_STALL;
    }
    F.n_blocks = n;
    return F.status = st;
}

// Stage 2, one block.
ZS_HD void parse_block(const uint8_t *zst, Block &B, uint32_t block_max) {
    if (B.type != 2 || B.status) return;
    // a compressed block of Block_Size >= Block_Maximum_Size would have been sent raw; the
    // format only bounds it by Block_Maximum_Size, which block_header checked
    B.status = parse_sections(zst + B.src, B.size, block_max, B.sec);
}

// Stage 3, one frame: who defines each block's tree and tables; arena bases within the frame.
ZS_HD void link_frame(Frame &F, Block *blocks) {
    if (F.status || F.skippable) return;
    uint32_t huf = NO_BLOCK, tab[3] = {NO_BLOCK, NO_BLOCK, NO_BLOCK};
    uint64_t lit = 0, seq = 0;
    for (uint32_t i = 0; i < F.n_blocks; ++i) {
        const uint32_t b = F.first_block + i;
        Block &B = blocks[b];
        if (B.status) {
            F.status = B.status;
            return;
        }
        if (B.type != 2) continue;
        if (B.sec.lit_type == 2) huf = b;
        if (B.sec.lit_type == 3 && huf == NO_BLOCK) B.status = E_HUF;
        B.huf_def = huf;
        if (B.sec.nseq) {
            for (uint32_t t = 0; t < 3; ++t) {
                if (B.sec.mode[t] != 3) tab[t] = b;
                if (tab[t] == NO_BLOCK) B.status = E_SEQHDR;  // a repeat with nothing to repeat
                B.tab_def[t] = tab[t];
            }
        }
        if (B.status) {
            F.status = B.status;
            return;
        }
        B.lit_base = (uint32_t)lit;
        B.seq_base = (uint32_t)seq;
        lit += B.sec.regen;
        seq += B.sec.nseq;
        if (lit >= (1ull << 32) || seq >= (1ull << 28)) {  // (a frame this large decodes to >= 4 GiB)
            F.status = B.status = E_SIZE;
            return;
        }
    }
    F.lit_total = (uint32_t)lit;
    F.seq_total = (uint32_t)seq;
}

// Stage 4: the Huffman table of one block (one lane) and its literal streams (k = 0 .. 3, one lane
// each); beside them its sequence tables and its sequences (one lane).
struct Tables {
    HufEntry huf[1 << HUF_MAX_BITS];
    FseEntry ll[1 << LL_MAX_LOG], of[1 << OF_MAX_LOG], ml[1 << ML_MAX_LOG];
    uint32_t huf_log, ll_log, of_log, ml_log;
    uint32_t soff[4], slen[4], doff[4], dlen[4];
    int32_t status, seq_status;  // of the literals half, of the sequences half
    Work w, w2;
};

// (the two halves touch disjoint parts of T: zstd.hip runs them in two waves)
ZS_HD void block_setup_literals(const uint8_t *zst, const Block *blocks, const Block &B, Tables &T) {
    T.status = OK;
    const Sections &s = B.sec;
    if (s.lit_type < 2) return;
    const Block &D = blocks[B.huf_def];
    T.status = huf_build(zst + D.src + D.sec.huf_desc, D.sec.huf_desc_len, T.huf, T.huf_log, T.w);
    if (!T.status) T.status = huf_split(zst + B.src + s.streams, s.streams_len, s.n_streams, s.regen, T.soff, T.slen, T.doff, T.dlen);
}

ZS_HD void block_setup_sequences(const uint8_t *zst, const Block *blocks, const Block &B, Tables &T) {
    T.seq_status = OK;
    if (!B.sec.nseq) return;
    for (uint32_t t = 0; t < 3 && !T.seq_status; ++t) {
        const Block &D = blocks[B.tab_def[t]];
        FseEntry *tab = t == 0 ? T.ll : t == 1 ? T.of : T.ml;
        uint32_t &log = t == 0 ? T.ll_log : t == 1 ? T.of_log : T.ml_log;
        T.seq_status = seq_table(t, D.sec.mode[t], zst + D.src + D.sec.tab[t], D.sec.tab_len[t], tab, log, T.w2);
    }
}

// lit: the block's extent of the literal arena, regen bytes
ZS_HD int32_t block_lit_stream(const uint8_t *zst, const Block &B, const Tables &T, uint32_t k, uint8_t *lit) {
    if (B.sec.lit_type < 2 || k >= B.sec.n_streams) return OK;
    if (T.doff[k] + T.dlen[k] > B.sec.regen) return E_LITHDR;
    return huf_stream(T.huf, T.huf_log, zst + B.src + B.sec.streams + T.soff[k], T.slen[k], lit + T.doff[k], T.dlen[k]);
}

// rec: the block's extent of the sequence arena, nseq records
ZS_HD int32_t block_sequences(const uint8_t *zst, Block &B, const Tables &T, uint32_t block_max, SeqRec *rec, uint32_t *stats) {
    B.map = rep_identity();
    if (B.sec.nseq == 0) {
        B.out_size = B.sec.regen;
        return OK;
    }
    return decode_sequences(zst + B.src + B.sec.bits, B.sec.bits_len, B.sec.nseq, T.ll, T.ll_log, T.of, T.of_log, T.ml,
                            T.ml_log, B.sec.regen, block_max, rec, B.map, B.out_size, stats);
}

// Stage 5, one frame: every block's incoming history and output base (within the frame).
ZS_HD void chain_frame(Frame &F, Block *blocks) {
    if (F.status || F.skippable) {
        F.out_size = 0;
        return;
    }
    uint32_t rep[3] = {1, 4, 8};
    uint64_t out = 0;
    for (uint32_t i = 0; i < F.n_blocks; ++i) {
        Block &B = blocks[F.first_block + i];
        if (B.status) {
            F.status = B.status;
            break;
        }
        for (int k = 0; k < 3; ++k) B.rep_in[k] = rep[k];
        B.out_base = (uint32_t)out;
        if (B.type != 2) B.out_size = B.rsize;
        out += B.out_size;
        if (out >= (1ull << 32)) {
            F.status = E_SIZE;
            break;
        }
        uint32_t nx[3];
        for (int k = 0; k < 3; ++k) nx[k] = rep_resolve(B.map.s[k], rep);
        for (int k = 0; k < 3; ++k) rep[k] = nx[k];
    }
    if (!F.status && F.has_fcs && F.fcs != out) F.status = E_SIZE;
    F.out_size = F.status ? 0 : (uint32_t)out;
}

}  // namespace zs
