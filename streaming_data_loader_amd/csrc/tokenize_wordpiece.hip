// tokenize_wordpiece.hip -- BERT WordPiece tokenization of a text arena on gfx950.
//
// Restates, for a whole arena of records at once, what the reference does one
// record at a time in TokenizerHolder::get_ids -> tokenizers::Tokenizer::encode
// (rust/src/tokenizer/tokenizer_holder.rs:19-28; crate tokenizers 0.13.1):
//   AddedVocabulary split (raw-text match of the added tokens)
//   -> BertNormalizer (clean_text, CJK padding; NFD + strip Mn and lowercase as the
//      tokenizer sets them: the Unicode table carries the setting, and the kernel's
//      CASED instantiation leaves ASCII letters as they are)
//   -> BertPreTokenizer (split on whitespace, isolate punctuation)
//   -> WordPiece (greedy longest-match-first, "##" continuation, 100-char cap).
// The template's [CLS]/[SEP] and the wrapper's framing are added at row
// assembly (pipeline.hip).
//
// One wave64 workgroup owns CHUNK = 1024 bytes of the arena; lane t owns
// bytes [c0 + 16t, c0 + 16t + 16):
//   1. each lane loads its 16 bytes with one 16-B non-temporal load (they stay
//      in VGPRs) and stores them into an LDS window [c0-32, c0+1024+32);
//      record starts in the window become an LDS bitmap;
//   2. classification is register-resident: an arithmetic ASCII classifier
//      packs 16 four-bit visible classes into one u64.  A lead byte >= 0xC0 is
//      looked up (two-level Unicode table in L2) by the lane that owns it and
//      its class goes into that lane's registers; the lane's first lead is
//      decoded from the window before the record bitmap exists, so its table
//      load is in flight together with the record offsets' loads.  Added-token
//      openers take a block-wide pass over an LDS list, which chunks without
//      an opener skip;
//   3. the state before the chunk comes from ballots over the 32 halo bytes
//      (the serial walk only when a non-ASCII byte or a possible added token
//      decides it), a wave scan carries the last visible class across lanes,
//      and piece starts (words, isolated chars, added tokens) are compacted
//      into an LDS list;
//   4. byte-level work is done once per byte, not once per piece: every lane
//      writes the 16 bits of its own bytes into two LDS bitmaps over the chunk
//      and 16 bytes of its right halo (wp_extent.hpp) -- S, where a run of
//      ASCII letters and digits stops (any other byte, a record start, the
//      text's end), and F, the stops a fast word may end at (ASCII whitespace
//      or punctuation, a non-ASCII whitespace / punctuation lead the rare pass
//      found, a record start, the text's end) -- from the classes of step 2.
//      Each lane then WordPiece-tokenizes pieces i, i+64, ...: a word's length
//      is a count of trailing zeros in S's window behind its first byte and
//      its fast flag one bit of F's, both windows from one LDS read; an ASCII
//      word of <= 16 bytes is read from LDS as 5 aligned dwords + v_alignbyte
//      and lower-cased by `| 0x20` under a byte mask (inside the length every
//      byte is a letter or digit).  Its first probe, the whole word, reads the
//      first-piece table (wp_first.hpp: the non-"##" pieces of <= 14 bytes in
//      16-byte slots, 1 MiB for a 30 K vocabulary): a three-multiply hash of its
//      4 dwords and two 16-B loads; a word that misses there or is longer goes to
//      the pending walk, where every candidate piece is one hash of 4 dwords +
//      one 32-B probe of the general vocab table whose slots hold the piece bytes
//      inline; other words take a general path (its byte buffers are LDS: the
//      kernel uses no scratch memory);
//   5. staged ids (LDS, indexed by piece byte position: a piece never has
//      more ids than bytes) are compacted into this chunk's slice of `tokc`
//      as a packed u16 list (STAGE slots a chunk), which the rows kernel reads
//      as it lies (pipeline.hip, list_index.hpp).  A slot holds an id where a
//      piece starts (the piece-start mask in the lane's registers) unless the
//      exception bitmap says otherwise -- a piece with more than one id, or
//      none (wp_pack.hpp).  A chunk without an exception bit (nearly every
//      chunk of in-vocabulary text) gathers its list through the piece
//      descriptors of step 3: entry e is the id staged at piece e's slot.  In
//      a chunk with exceptions lane t packs its own 16 slots, a slot's list
//      position a wave sum plus a popcount.  Each record boundary's local id
//      offset comes from the same sums, fetched from the owning lane by a shuffle.
#include "common.hpp"
#include "device_util.hpp"
#include "kernels.hpp"
#include "tok_device.hpp"
#include "wp_extent.hpp"
#include "wp_pack.hpp"

#include <cstdio>

namespace sdl {

namespace {

// ASCII visible class (same as the table's ASCII rows; checked on the host)
__device__ __forceinline__ uint32_t ascii_vclass(uint32_t b) {
    const uint32_t l = b | 0x20u;
    if (l - 'a' < 26u || b - '0' < 10u) return V_OTHER;
    if (b == ' ' || b == '\t' || b == '\n' || b == '\r') return V_WS;
    if (b < 32u || b == 127u) return V_NONE;
    return V_ISO;
}

// ascii_vclass of 4 bytes as 4 nibbles (bytes >= 0x80: V_NONE)
__device__ __forceinline__ uint32_t vclass4(uint32_t x) {
    const uint32_t lo7 = ~x & B7, a = x & 0x7F7F7F7Fu;
    const uint32_t an = swar_alnum(x);
    const uint32_t ws = (in7(a, 9, 10) | in7(a, 13, 13) | in7(a, ' ', ' ')) & lo7;
    const uint32_t ctl = ~ge7(a, 32) | ge7(a, 127);  // includes \t \n \r (ws wins)
    const uint32_t iso = lo7 & ~an & ~ws & ~ctl;
    return nibpack4(((an | ws) >> 7) | ((an | iso) >> 6));  // OTHER 3, WS 1, ISO 2, NONE 0
}

// Device Unicode entry (assets.cpp: device_entry): bits 0-1 class, bit 2
// identity, bit 3 inline (bits 4-5 nbytes-1, 6-7 nchars-1, 8-31 the bytes),
// else bits 8-31 = pool offset.  One load for the BMP, two beyond it.
__device__ __forceinline__ uint32_t uentry(const DevTok &T, uint32_t cp) {
    if (cp < 0x10000u) return T.ubmp[cp].x;
    if (cp >= 0x110000u) return UC_DEL;
    return T.uentry[(uint32_t)T.upage[cp >> 7] * 128u + (cp & 127u)];
}
__device__ __forceinline__ int entry_nchars(const DevTok &T, uint32_t e) {
    if (e & 4u) return 1;
    if (e & 8u) return (int)((e >> 6) & 3u) + 1;
    return T.upool[(e >> 8) + 1];
}

__device__ __forceinline__ uint32_t vclass_of_entry(uint32_t e) {
    switch (e & 3u) {
        case UC_OTHER: return V_OTHER;
        case UC_WS: return V_WS;
        case UC_ISO: return V_ISO;
        default: return V_NONE;
    }
}

// decode() of the char at window index wi (arena position p) before the record-start bitmap
// exists: the same result unless a record starts inside the sequence, which the caller
// checks once it does.
__device__ __forceinline__ uint32_t decode_spec(const lds_u8 *win, int wi, int64_t p, int64_t N, int *len) {
    const uint32_t b = win[wi];
    int n;
    uint32_t c;
    if ((b & 0xE0u) == 0xC0u) { n = 2; c = b & 0x1Fu; }
    else if ((b & 0xF0u) == 0xE0u) { n = 3; c = b & 0x0Fu; }
    else if ((b & 0xF8u) == 0xF0u) { n = 4; c = b & 0x07u; }
    else { *len = 1; return 0xFFFDu; }
    if (p + n > N) { *len = 1; return 0xFFFDu; }
    for (int k = 1; k < n; ++k) {
        const uint32_t x = win[wi + k];
        if ((x & 0xC0u) != 0x80u) { *len = 1; return 0xFFFDu; }
        c = (c << 6) | (x & 0x3Fu);
    }
    *len = n;
    return c;
}
// Entry of a decoded char and, for a canonical BMP char, its precomputed one-char id in one load.
__device__ __forceinline__ uint2 uentry2(const DevTok &T, uint32_t cp, int len) {
    return (len == 2 && cp >= 0x80u) || (len == 3 && cp >= 0x800u) ? T.ubmp[cp] : make_uint2(uentry(T, cp), 0u);
}

// Full visible class of the char at q (general path).
__device__ __forceinline__ uint32_t vclass_general(const Ctx &C, int64_t q) {
    const DevTok &T = *C.T;
    const uint32_t b = C.byte(q);
    if ((b & 0xC0u) == 0x80u) return V_NONE;
    if (T.n_special) {
        for (int d = 1; d < T.max_special_len; ++d) {  // covered by an earlier added token?
            if (C.rstart(q - d + 1)) break;
            const int64_t x = q - d;
            if (x < 0) break;
            if (C.byte(x) == T.opener) {
                const int m = special_match(C, x);
                if (m >= 0 && T.special_len[m] > d) return V_NONE;
                break;
            }
        }
        if (b == T.opener && special_match(C, q) >= 0) return V_SPEC;
    }
    if (b < 0x80u) return ascii_vclass(b);
    int len;
    return vclass_of_entry(uentry(T, decode(C, q, b, &len)));
}

// ---- WordPiece ------------------------------------------------------------------

// WordPiece::tokenize over a normalized word held in a byte buffer (LDS).
template <typename Buf>
__device__ __forceinline__ int wordpiece_general(const DevTok &T, const Buf *w, int L, lds_u16 *out) {
    int n = 0, start = 0;
    while (start < L) {
        const int lim = start == 0 ? T.maxlen_first : T.maxlen_cont;
        int end = start + lim < L ? start + lim : L;
        while (end < L && end > start && (w[end] & 0xC0) == 0x80) --end;
        int id = -1;
        while (end > start) {
            id = probe_general(T, w, start, end, start > 0 ? 1u : 0u);
            if (id >= 0) break;
            do { --end; } while (end > start && (w[end] & 0xC0) == 0x80);
        }
        if (id < 0) {
            out[0] = (uint16_t)T.unk_id;
            return 1;
        }
        out[n++] = (uint16_t)id;
        start = end;
    }
    return n;
}

// Appends the normalized bytes of a non-ASCII OTHER/ISO char.
template <typename Buf>
__device__ __forceinline__ int append_norm(const Ctx &C, uint32_t e, int64_t p, int len, Buf *buf, int nb) {
    if (e & 4u) {
        for (int k = 0; k < len; ++k) buf[nb + k] = (uint8_t)C.byte(p + k);
        return nb + len;
    }
    if (e & 8u) {
        const int m = (int)((e >> 4) & 3u) + 1;
        for (int k = 0; k < m; ++k) buf[nb + k] = (uint8_t)(e >> (8 + 8 * k));
        return nb + m;
    }
    const uint8_t *pe = C.T->upool + (e >> 8);
    const int m = pe[0];
    for (int k = 0; k < m; ++k) buf[nb + k] = pe[2 + k];
    return nb + m;
}

__device__ __forceinline__ int utf8_len(uint32_t lead) {
    return lead < 0x80u ? 1 : (lead & 0xE0u) == 0xC0u ? 2 : (lead & 0xF0u) == 0xE0u ? 3 : 4;
}

// Extent of the general WORD piece at p: it runs over OTHER and invisible
// chars until a WS/ISO char, an added token or the record end.  Counts its
// normalized chars (stops past MAX_WORD_CHARS) and bytes.
__device__ __forceinline__ int64_t word_extent(const Ctx &C, int64_t p, int64_t rec_end, int *nchars_out, int *nbytes_out) {
    const DevTok &T = *C.T;
    int64_t i = p;
    int nchars = 0, nbytes = 0;
    while (i < rec_end && nchars <= MAX_WORD_CHARS) {
        const uint32_t b = C.byte(i);
        if (b < 0x80u) {
            const uint32_t c = ascii_vclass(b);
            if (c == V_OTHER) {
                if (T.n_special && b == T.opener && special_match(C, i) >= 0) break;
                ++nchars;
                ++nbytes;
                ++i;
                continue;
            }
            if (c == V_NONE) { ++i; continue; }
            break;
        }
        if ((b & 0xC0u) == 0x80u) { ++i; continue; }
        int len;
        const uint32_t e = uentry(T, decode(C, i, b, &len));
        const uint32_t c = e & 3u;
        if (c == UC_OTHER) {
            nchars += entry_nchars(T, e);
            nbytes += (e & 4u) ? len : (e & 8u) ? (int)((e >> 4) & 3u) + 1 : (int)T.upool[e >> 8];
        } else if (c != UC_DEL) {
            break;
        }
        i += len;
    }
    *nchars_out = nchars;
    *nbytes_out = nbytes;
    return i;
}

// Normalized bytes of the word [p, i) into buf (private or LDS); returns the
// count.  NFD canonical ordering of the kept combining marks: a run of them is
// appended as it comes and sorted in place (stable, by ccc) when a starter --
// kept, removed or inside a precomposed char -- ends it.  CASED: the normalizer keeps
// case, so an ASCII letter goes in as it is (every other char's form is the table's).
template <bool CASED, typename Buf>
__device__ __forceinline__ int word_materialize(const Ctx &C, int64_t p, int64_t i, Buf *buf) {
    const DevTok &T = *C.T;
    int nb = 0;
    int run = -1;
    auto ccc_at = [&](int x, int l) {
        uint32_t cp = l == 2 ? buf[x] & 0x1Fu : l == 3 ? buf[x] & 0x0Fu : buf[x] & 0x07u;
        for (int k = 1; k < l; ++k) cp = (cp << 6) | (buf[x + k] & 0x3Fu);
        return (uentry(T, cp) >> 8) & 0xFFu;
    };
    auto flush = [&]() {
        if (run < 0) return;
        for (bool swapped = true; swapped;) {
            swapped = false;
            for (int x = run; x < nb;) {
                const int l1 = utf8_len(buf[x]);
                if (x + l1 >= nb) break;
                const int l2 = utf8_len(buf[x + l1]);
                if (ccc_at(x, l1) > ccc_at(x + l1, l2)) {
                    uint32_t t = 0;  // (a char is at most 4 bytes)
                    for (int k = 0; k < l1; ++k) t |= (uint32_t)buf[x + k] << (8 * k);
                    for (int k = 0; k < l2; ++k) buf[x + k] = buf[x + l1 + k];
                    for (int k = 0; k < l1; ++k) buf[x + l2 + k] = (uint8_t)(t >> (8 * k));
                    swapped = true;
                    x += l2;
                } else {
                    x += l1;
                }
            }
        }
        run = -1;
    };
    auto push = [&](uint32_t bytes, int l) {
        if (run < 0) run = nb;
        for (int k = 0; k < l; ++k) buf[nb++] = (uint8_t)(bytes >> (8 * k));
    };
    for (int64_t q = p; q < i;) {
        const uint32_t b = C.byte(q);
        if (b < 0x80u) {
            if (ascii_vclass(b) == V_OTHER) {
                flush();
                buf[nb++] = (uint8_t)((!CASED && b - 'A' < 26u) ? b + 32u : b);
            }
            ++q;
            continue;
        }
        if ((b & 0xC0u) == 0x80u) { ++q; continue; }
        int len;
        const uint32_t e = uentry(T, decode(C, q, b, &len));
        const uint32_t cls = e & 3u;
        if ((e & 24u) == 16u) {  // canonical ordering entry
            if (cls == UC_DEL) {
                flush();  // a removed starter ends the run
            } else if (e & 4u) {  // a kept mark
                uint32_t bytes = 0;
                for (int k = 0; k < len; ++k) bytes |= C.byte(q + k) << (8 * k);
                push(bytes, len);
            } else {  // precomposed: its starters end the run, its kept marks join it
                const uint8_t *pe = T.upool + (e >> 8);
                const int m = pe[0];
                for (int x = 0; x < m;) {
                    const uint32_t lead = pe[2 + x];
                    const int l = utf8_len(lead);
                    uint32_t cp = l == 1 ? lead : l == 2 ? lead & 0x1Fu : l == 3 ? lead & 0x0Fu : lead & 0x07u;
                    uint32_t bytes = lead;
                    for (int k = 1; k < l; ++k) {
                        cp = (cp << 6) | (pe[2 + x + k] & 0x3Fu);
                        bytes |= (uint32_t)pe[2 + x + k] << (8 * k);
                    }
                    const uint32_t e2 = uentry(T, cp);
                    if ((e2 & 24u) == 16u && (e2 & 4u) && (e2 & 3u) == UC_OTHER) {
                        push(bytes, l);
                    } else {
                        flush();
                        for (int k = 0; k < l; ++k) buf[nb++] = (uint8_t)(bytes >> (8 * k));
                    }
                    x += l;
                }
            }
        } else if (cls == UC_OTHER) {
            flush();
            nb = append_norm(C, e, q, len, buf, nb);
        }
        q += len;
    }
    flush();
    return nb;
}

// General WORD piece [p, i) of at most MAX_WORD_CHARS normalized chars, materialized in
// `buf` (LDS, MAX_WORD_BYTES), WordPiece one probe at a time (words whose normalization
// exceeds the lattice's LW_MAX bytes).
template <bool CASED>
__device__ __forceinline__ int word_general(const Ctx &C, int64_t p, int64_t i, lds_u8 *buf, lds_u16 *out) {
    const int nb = word_materialize<CASED>(C, p, i, buf);
    return wordpiece_general(*C.T, buf, nb, out);
}

// Bytes [off, off + 16) of an LDS byte buffer (dword aligned, readable 20
// bytes past off) in registers, the first n kept.
__device__ __forceinline__ W16 lds_w16(const lds_u32 *b32, int off, int n) {
    const int a = off >> 2;
    const uint32_t sh = (uint32_t)(off & 3);
    const uint32_t x0 = b32[a], x1 = b32[a + 1], x2 = b32[a + 2], x3 = b32[a + 3], x4 = b32[a + 4];
    return keep_bytes(W16{__builtin_amdgcn_alignbyte(x1, x0, sh), __builtin_amdgcn_alignbyte(x2, x1, sh),
                          __builtin_amdgcn_alignbyte(x3, x2, sh), __builtin_amdgcn_alignbyte(x4, x3, sh)},
                      n < 16 ? n : 16);
}

// start of the char that ends right before byte `end` (UTF-8 in registers)
__device__ __forceinline__ int w16_prev_char(const W16 &w, int end, int start) {
    int e = end - 1;
    while (e > start && (w16_byte(w, e) & 0xC0u) == 0x80u) --e;
    return e;
}

// BertNormalizer output of the WORD piece at p (or of the single ISO char at
// p if iso) into registers.  Returns false if the normalized word does not fit
// in 16 bytes (then the scratch path handles it, including the 100-char rule).
template <bool CASED>
__device__ __forceinline__ bool normalize_w16(const Ctx &C, int64_t p, int64_t rec_end, bool iso, W16 &w, int &L) {
    const DevTok &T = *C.T;
    w = W16{0, 0, 0, 0};
    int nb = 0;
    int64_t i = p;
    while (i < rec_end) {
        const uint32_t b = C.byte(i);
        if (b < 0x80u) {
            const uint32_t c = ascii_vclass(b);
            if (iso || c == V_OTHER) {
                if (!iso && T.n_special && b == T.opener && special_match(C, i) >= 0) break;
                if (nb >= 16) return false;
                w16_put(w, nb++, (!CASED && b - 'A' < 26u) ? b + 32u : b);
                ++i;
                if (iso) break;
                continue;
            }
            if (c == V_NONE) { ++i; continue; }
            break;
        }
        if ((b & 0xC0u) == 0x80u) { ++i; continue; }
        int len;
        const uint32_t e = uentry(T, decode(C, i, b, &len));
        const uint32_t c = e & 3u;
        if (c == UC_OTHER && (e & 24u) == 16u) return false;  // canonical ordering: the general path
        if (iso || c == UC_OTHER) {
            if (e & 4u) {
                if (nb + len > 16) return false;
                for (int k = 0; k < len; ++k) w16_put(w, nb++, C.byte(i + k));
            } else if (e & 8u) {
                const int m = (int)((e >> 4) & 3u) + 1;
                if (nb + m > 16) return false;
                for (int k = 0; k < m; ++k) w16_put(w, nb++, (e >> (8 + 8 * k)) & 0xFFu);
            } else {
                const uint8_t *pe = T.upool + (e >> 8);
                const int m = pe[0];
                if (nb + m > 16) return false;
                for (int k = 0; k < m; ++k) w16_put(w, nb++, pe[2 + k]);
            }
            i += len;
            if (iso) break;
            continue;
        }
        if (c == UC_DEL) { i += len; continue; }
        break;
    }
    L = nb;
    return true;
}

// Record end (first record start > p, p in the window) for the general paths:
// the next bit of the window's record-start bitmap, else the first start past
// the window (rb_next).
__device__ __forceinline__ int64_t rec_end_of(const Ctx &C, int64_t rb_next, int64_t p) {
    const int b = (int)(p - C.w0) + 1;
    for (int wd = b >> 5; wd < RBITS_WORDS; ++wd) {
        uint32_t m = C.rbits[wd];
        if (wd == (b >> 5)) m &= ~0u << (b & 31);
        if (m) return C.w0 + 32 * wd + __builtin_ctz(m);
    }
    return rb_next;
}

}  // namespace

// Diagnostic build (-DSDL_STAMPS): wave 0 of every block adds the s_memtime
// cycles spent between phase boundaries (each right after a barrier) into
// sdl_phase_cycles[]; the host prints them.  Never compiled into the product.
#ifdef SDL_STAMPS
__device__ unsigned long long sdl_phase_cycles[16];
#define PHASE_STAMP(k)                                                                  \
    do {                                                                              \
        if (threadIdx.x == 0) {                                                       \
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();              \
            atomicAdd(&sdl_phase_cycles[k], t_ - stamp_prev_);                        \
            stamp_prev_ = t_;                                                         \
        }                                                                             \
    } while (0)
#else
#define PHASE_STAMP(k) \
    do {             \
    } while (0)
#endif

// Waves per SIMD the register budget is cut to: 5 (96 VGPRs).  6 (80 VGPRs)
// was 1% faster before the deferred-word lattice; with it, 80 VGPRs spill and
// 5 measures faster on both corpora (fixture 1.868 -> 1.818 ms, held-out
// 2.98 -> 2.86 ms).  LDS (7.1 KB per one-wave block) admits ~5.5 anyway; one
// more 64-B array (7.7 KB) cost 7%.
constexpr int WP_WAVES = 5;
// candidate lengths the pending-word state machine probes per step (longest
// first).  3 and 4 were measured: parity-green and no faster (4: 96 VGPRs,
// fixture 1.14 -> 1.19 ms, held-out 2.32 -> 2.40; 3: within noise) -- the
// machine is bound by its lanes' probe latency, not by its step count.
constexpr int WP_NPROBE = 2;
// CASED: the tokenizer's BertNormalizer keeps case (lowercase=false).  A compile-time variant,
// not a field of DevTok or DevFirst (their layout is shared with the BPE and Unigram kernels):
// the uncased instantiation is the kernel as it was, and the cased one drops the lower-casing
// of ASCII letters at its three sites -- word_setup, normalize_w16, word_materialize.
template <bool CASED>
__global__ __launch_bounds__(TOK_THREADS) __attribute__((amdgpu_waves_per_eu(WP_WAVES, 8))) void k_wordpiece_chunks(
    DevTok T, DevFirst F, const uint8_t *__restrict__ text, int64_t N, const uint64_t *__restrict__ off, int64_t R,
    const uint32_t *__restrict__ ranges, uint16_t *__restrict__ tokc, uint32_t *__restrict__ chunk_cnt,
    uint32_t *__restrict__ rec_local, int64_t c_begin) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[WIN];
    __shared__ uint32_t s_rbits[RBITS_WORDS + 1];
    __shared__ __attribute__((aligned(16))) uint16_t s_pieces[CHUNK];   // (pos - c0) | kind << 12
    __shared__ __attribute__((aligned(16))) uint16_t s_stage[STAGE];  // ids staged at their piece's byte position
    // per-byte class overrides of the rare pass (step 2); from step 4 on its first words are the
    // exception bitmap of the stage slots (wp_pack.hpp) and, behind it, the stop and
    // fast-terminator bitmaps of the chunk's bytes (wp_extent.hpp)
    __shared__ __attribute__((aligned(16))) uint8_t s_ovr[CHUNK];
    __shared__ uint16_t s_pend[PEND_CAP];  // pending piece indices (step 4b)
    __shared__ uint32_t s_scratch[TOK_THREADS / 64 + 3];
    // non-ASCII chars found by the rare pass: [0, 32) a WS/ISO char starts at the
    // chunk position (a word before it ends there), [32, 64) an ISO char whose id
    // is already in its stage slot
    __shared__ uint32_t s_nabits[2 * CHUNK / 32];

    const int tid = threadIdx.x;
#ifdef SDL_STAMPS
    unsigned long long stamp_prev_ = __builtin_amdgcn_s_memtime();
#endif
    const int64_t ci = c_begin + xcd_chunk();  // this block's chunk
    const int64_t c0 = ci * CHUNK;
    const int64_t c1 = c0 + CHUNK < N ? c0 + CHUNK : N;
    const int64_t w0 = c0 - HALO_L;
    const lds_u8 *win = (const lds_u8 *)s_win;
    const lds_u32 *rbits = (const lds_u32 *)s_rbits;

    // ---- 1. load -------------------------------------------------------------
    const uint4 v = load16(text, c0 + 16 * tid, N);
    uint4 hv = make_uint4(0u, 0u, 0u, 0u);
    int64_t hp = 0;
    if (tid < (WIN - CHUNK) / 16) {  // left and right halo pieces
        hp = tid < HALO_L / 16 ? w0 + 16 * tid : c0 + CHUNK + 16 * (tid - HALO_L / 16);
        hv = load16(text, hp, N);
    }
    const int64_t ra = ranges[3 * ci], rz = ranges[3 * ci + 1], r_lo = ranges[3 * ci + 2];
    *reinterpret_cast<uint4 *>(s_win + HALO_L + 16 * tid) = v;
    if (tid < (WIN - CHUNK) / 16) *reinterpret_cast<uint4 *>(s_win + (hp - w0)) = hv;
    if (tid <= RBITS_WORDS) s_rbits[tid] = 0;
    s_nabits[tid] = 0u;  // 2 * CHUNK / 32 == TOK_THREADS words
    const int nrb = (int)(rz - ra);
    int64_t rb_next = rz <= R ? (int64_t)off[rz] : N;
    if (rb_next > N) rb_next = N;
    __syncthreads();
    // ---- 2. register-resident classification of the lane's 16 bytes ----------
    // (before the record-start bitmap, which only the lookups after it need)
    const int64_t s0 = c0 + 16 * tid;
    const int nown = s0 >= c1 ? 0 : (int)(c1 - s0 < 16 ? c1 - s0 : 16);
    const int rel0 = HALO_L + 16 * tid;  // window index of s0 (multiple of 16)
    const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
    uint64_t cls = 0;
    uint32_t leads = 0, opens = 0;
    // the ASCII classes step 4's bitmaps need, kept from here (one register; classifying the 16
    // bytes again there costs more): bits 0-15 WS or ISO, 16-31 letter or digit
    uint32_t sfm = 0;
    static_assert(V_OTHER == WX_V_OTHER && V_WS == WX_V_WS && V_ISO == WX_V_ISO && V_NONE == 0, "");
    const uint32_t o4 = T.opener * 0x01010101u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t x = wv[j];
        const uint32_t n4 = vclass4(x);
        cls |= (uint64_t)n4 << (16 * j);
        sfm |= wx_nibble_classes(n4) << (4 * j);
        leads |= gather4(x & (x << 1)) << (4 * j);  // >= 0xC0
        opens |= gather4(~nzb(x ^ o4)) << (4 * j);
    }
    if (!T.n_special) opens = 0;
    if (nown < 16) {
        cls &= nown ? ((1ull << (4 * nown)) - 1ull) : 0ull;
        leads &= (1u << nown) - 1u;
        opens &= (1u << nown) - 1u;
    }
    // Non-ASCII lead bytes (rare: a few a KiB of English text) are looked up by the lane that
    // owns them: decode + two-level Unicode table, the class goes into the lane's own `cls`.
    // The lane's first lead is decoded here, from the window alone, so that its table load is
    // in flight together with the record offsets' loads below and not after their barrier.
    const int l0 = leads ? __builtin_ctz(leads) : -1;
    uint2 ue0 = make_uint2(0u, 0u);
    int len0 = 1;
    if (l0 >= 0) {
        const uint32_t cp0 = decode_spec(win, rel0 + l0, s0 + l0, N, &len0);
        ue0 = uentry2(T, cp0, len0);
    }
    for (int k = tid; k < nrb; k += TOK_THREADS) {
        const int rel = (int)((int64_t)off[ra + k] - w0);
        atomicOr(&s_rbits[rel >> 5], 1u << (rel & 31));
    }
    __syncthreads();
    PHASE_STAMP(1);

    const Ctx C{&T, win, rbits, w0, text, N, off, R};
#ifdef SDL_ABLATE
    // diagnostic build (tools/build_variants.py abl3=SDL_ABLATE, tools/pmc_calibration.py): load only; every record gets 0 ids (so later stages stay in bounds)
    {  // (an opaque use of the window keeps its loads: `x & 0u` let the compiler drop them all)
        const uint32_t x = s_win[HALO_L + (ci & 1023)];
        asm volatile("" ::"v"(x));
    }
    if (tid == 0) chunk_cnt[ci] = 0u;
    for (int64_t r = r_lo + tid; r <= R && (int64_t)off[r] < c1; r += TOK_THREADS) rec_local[r] = 0;
    return;
#endif

    // record starts at the lane's bytes and the 16 after them
    const uint32_t rm32 = (uint32_t)((((uint64_t)rbits[(rel0 >> 5) + 1] << 32) | rbits[rel0 >> 5]) >> (rel0 & 31));
    const uint32_t rmask = rm32 & 0xFFFFu;
    for (uint32_t m = leads; m; m &= m - 1) {
        const int i = __builtin_ctz(m);
        const int wi = rel0 + i, rel = 16 * tid + i;
        int len = len0;
        uint2 ue = ue0;
        // every other lead, and a first lead with a record start inside its sequence (never in
        // valid text), through the checked decode
        if (i != l0 || ((rm32 >> (i + 1)) & ((1u << (len0 - 1)) - 1u)) != 0u) {
            const uint32_t cp = decode(C, w0 + wi, win[wi], &len);
            ue = uentry2(T, cp, len);
        }
        const uint32_t e = ue.x;
        const uint32_t vc = vclass_of_entry(e);
        cls = (cls & ~(0xFull << (4 * i))) | ((uint64_t)vc << (4 * i));
        if (vc == V_WS || vc == V_ISO) atomicOr(&s_nabits[rel >> 5], 1u << (rel & 31));
        // an ISO char is a piece of its own: when it normalizes to one char of <= 16
        // bytes, its WordPiece is one probe of that char (no "##" piece can start
        // inside a char), done here so the piece skips the pending pass
        if (ue.y >> 31) {
            s_stage[rel] = (uint16_t)ue.y;
            atomicOr(&s_nabits[CHUNK / 32 + (rel >> 5)], 1u << (rel & 31));
        } else if (vc == V_ISO && (e & 24u) != 16u && ((e & 4u) || ((e & 8u) && ((e >> 6) & 3u) == 0u))) {
            W16 w{0, 0, 0, 0};
            int L;
            if (e & 4u) {
                L = len;
                for (int q = 0; q < len; ++q) w16_put(w, q, win[wi + q]);
            } else {
                L = (int)((e >> 4) & 3u) + 1;
                for (int q = 0; q < L; ++q) w16_put(w, q, (e >> (8 + 8 * q)) & 0xFFu);
            }
            const int id = L <= T.maxlen_first ? probe_result(probe_load(T, hash16(w, (uint32_t)L, 0u)), (uint32_t)L, w)
                                               : -1;
            s_stage[rel] = (uint16_t)(id >= 0 ? id : T.unk_id);
            atomicOr(&s_nabits[CHUNK / 32 + (rel >> 5)], 1u << (rel & 31));
        }
    }
    PHASE_STAMP(12);
    // Added tokens: every opener byte that starts a match marks its bytes (SPEC at the start,
    // invisible after) as per-byte class overrides in LDS, one opener per thread from a work
    // list in s_pieces (free until the pieces are found); applied after the leads' classes.
    // tid 0 also owns openers in [c0 - max_special_len + 1, c0) (a ballot over the halo's
    // bytes): a token starting there may cover this chunk's first bytes.  Chunks without an opener skip all of it.
    static_assert(TOK_THREADS == 64, "__any() is the block's vote");
    // the left halo, lane j < 32: byte c0 - 1 - j (also the look-back's, below)
    const bool in_halo = tid < HALO_L;
    const uint32_t hb = in_halo ? win[HALO_L - 1 - tid] : 0u;
    const uint64_t halo_open = T.n_special ? __ballot(in_halo && hb == T.opener) : 0ull;
    const uint32_t opens_left =
        tid == 0 && T.max_special_len > 1 ? (uint32_t)halo_open & ((1u << (T.max_special_len - 1)) - 1u) : 0u;
    static_assert(MAX_SPECIAL_LEN <= HALO_L, "an added token that covers the chunk's first byte starts in the halo");
    if (__any((opens | opens_left) != 0u)) {
        *reinterpret_cast<uint4 *>(s_ovr + 16 * tid) = make_uint4(~0u, ~0u, ~0u, ~0u);
        uint32_t n_opens;
        uint32_t ob = block_excl_sum<TOK_THREADS>((uint32_t)(__builtin_popcount(opens) + __builtin_popcount(opens_left)),
                                                  &n_opens, s_scratch);
        for (uint32_t m = opens; m; m &= m - 1) s_pieces[ob++] = (uint16_t)(rel0 + __builtin_ctz(m));
        for (uint32_t m = opens_left; m; m &= m - 1) s_pieces[ob++] = (uint16_t)(HALO_L - (__builtin_ctz(m) + 1));
        __syncthreads();
        PHASE_STAMP(2);
        for (uint32_t k = tid; k < n_opens; k += TOK_THREADS) {
            const int wi = s_pieces[k];
            const int64_t x = w0 + wi;
            const int m = special_match(C, x);
            if (m < 0) continue;
            const int l = T.special_len[m];
            for (int j = 0; j < l; ++j) {
                const int64_t y = x + j;
                if (y >= c0 && y < c1) s_ovr[y - c0] = (uint8_t)(j == 0 ? V_SPEC : V_NONE);
            }
        }
        __syncthreads();
        const uint4 o = *reinterpret_cast<const uint4 *>(s_ovr + 16 * tid);
        const uint32_t ov[4] = {o.x, o.y, o.z, o.w};
        uint64_t onib = 0, keep = 0;  // override classes, nibbles without one (0xFF)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            onib |= (uint64_t)nibpack4(ov[j] & 0x0F0F0F0Fu) << (16 * j);
            keep |= (uint64_t)nibpack4(fullb(ov[j] & B7) & 0x0F0F0F0Fu) << (16 * j);
        }
        cls = (cls & keep) | (onib & ~keep);
    }
    PHASE_STAMP(3);
    // Each byte's previous visible class, byte-parallel: a record start at byte
    // i + 1 puts a stopper (8) at byte i, then the visible classes and stoppers
    // fill forward over the invisible bytes in four doubling steps.
    constexpr uint64_t NIB1 = 0x1111111111111111ull;
    auto nib_zero = [](uint64_t x) -> uint64_t {  // 1 at the base bit of every zero nibble
        return ~(x | (x >> 1) | (x >> 2) | (x >> 3)) & NIB1;
    };
    const uint64_t stop = nib_spread(rmask >> 1);
    uint64_t fill = (cls & ~((stop << 4) - stop)) | (stop << 3);
#pragma unroll
    for (int sh = 4; sh < 64; sh <<= 1) {
        const uint64_t z = nib_zero(fill);
        fill |= (fill << sh) & ((z << 4) - z);
    }
    // lane summary for the carry scan: 0 = pass-through, 0x100 | v = state after
    const uint32_t last = (uint32_t)(fill >> 60);
    const uint32_t summ = (last != 0u || (rmask & 1u)) ? 0x100u | (last & 7u) : 0u;
    // state before the chunk: last visible char of the same record before c0.  Lanes 0-31
    // each take one byte of the left halo (lane j: byte c0 - 1 - j); ballots give the visible
    // ASCII bytes, the record starts and the bytes only the general classifier can judge -- a
    // byte >= 0x80, or one an added token could cover or start: an opener at it or within
    // max_special_len - 1 bytes before it, or that range leaving the halo.  The state is the
    // class of the nearest visible byte unless a record start comes first; a general byte in
    // the deciding range, or a halo without either, takes the serial walk (wave-uniform).
    uint32_t chunk_state;
    {
        const uint32_t hvc = ascii_vclass(hb & 0x7Fu);
        const int ri = HALO_L - (in_halo ? tid : 0);  // window index of the byte after
        const uint64_t rsm = __ballot(in_halo && ((rbits[ri >> 5] >> (ri & 31)) & 1u));
        const uint64_t vism = __ballot(in_halo && hb < 0x80u && hvc != V_NONE);
        uint64_t gen = __ballot(in_halo && hb >= 0x80u);
        if (T.n_special) {
            const int msl = T.max_special_len;
            for (int d = 0; d < msl && d < HALO_L; ++d) gen |= halo_open >> d;
            gen |= msl > HALO_L ? ~0ull : ~0ull << (HALO_L + 1 - msl);
        }
        const int jr = rsm ? __builtin_ctzll(rsm) : 64, jv = vism ? __builtin_ctzll(vism) : 64;
        bool fast;
        if (jr <= jv) {  // a record start ends the search before anything visible
            fast = jr < 64 && (gen & ((1ull << jr) - 1ull)) == 0ull;
            chunk_state = V_NONE;
        } else {
            fast = (gen & ((2ull << jv) - 1ull)) == 0ull;
            chunk_state = lane_bcast(hvc, jv);
        }
        if (!fast) {
            if (tid == 0) {
                uint32_t st = V_NONE;
                int64_t q = c0 - 1;
                while (q >= 0 && !C.rstart(q + 1)) {
                    int64_t cs = q;
                    int k = 0;
                    while (k < 3 && cs > 0 && (C.byte(cs) & 0xC0u) == 0x80u && !C.rstart(cs)) { --cs; ++k; }
                    const uint32_t vc = vclass_general(C, cs);
                    if (vc != V_NONE) { st = vc; break; }
                    q = cs - 1;
                }
                s_scratch[TOK_THREADS / 64] = st;
            }
            __syncthreads();
            chunk_state = s_scratch[TOK_THREADS / 64];
            __syncthreads();
        }
    }
    PHASE_STAMP(4);
    const uint32_t st_in = block_excl_last_scan<TOK_THREADS>(summ, s_scratch);

    // ---- 3. piece starts -------------------------------------------------------
    uint32_t pmask;
    {
        const uint32_t st = (rmask & 1u) ? (uint32_t)V_NONE : (st_in & 0x100u) ? (st_in & 0xFFu) : chunk_state;
        uint64_t pv = fill << 4;  // previous visible class (stopper 8: none)
        const uint64_t z = nib_zero(pv);  // nothing visible before in the lane: the incoming state
        pv = (pv | (((z << 4) - z) & (NIB1 * st))) & 0x7777777777777777ull;
        const uint64_t is_o = nib_zero(cls ^ (NIB1 * V_OTHER));
        const uint64_t is_si = nib_zero(cls ^ (NIB1 * V_ISO)) | nib_zero(cls ^ (NIB1 * V_SPEC));
        uint64_t m = (is_si | (is_o & ~nib_zero(pv ^ (NIB1 * V_OTHER)))) & NIB1;  // bit 4i: a piece starts at byte i
        m = (m | (m >> 3)) & 0x0303030303030303ull;
        m = (m | (m >> 6)) & 0x000F000F000F000Full;
        m = (m | (m >> 12)) & 0x000000FF000000FFull;
        pmask = (uint32_t)((m | (m >> 24)) & 0xFFFFull);
    }
    uint32_t np_total;
    uint32_t pbase = block_excl_sum<TOK_THREADS>((uint32_t)__builtin_popcount(pmask), &np_total, s_scratch);
    for (uint32_t m = pmask; m;) {
        const int i = __builtin_ctz(m);
        m &= m - 1;
        const uint32_t c = (uint32_t)(cls >> (4 * i)) & 0xFu;
        s_pieces[pbase++] = (uint16_t)((16 * tid + i) | (c << 12));
    }
    __syncthreads();
    PHASE_STAMP(5);
    const int np = (int)np_total;

    // ---- 4. tokenize pieces ---------------------------------------------------------
    // (a) every lane sets up TOK_UNROLL pieces at a time and issues their
    //     full-word probes of the first-piece table back to back, so most words
    //     (in-vocabulary, <= 14 B) finish with one latency and 2 * TOK_UNROLL
    //     loads in flight per lane -- all of a chunk's first probes in one
    //     flight unless it holds more than TOK_THREADS * TOK_UNROLL pieces;
    //     added tokens and one-byte punctuation finish without a probe;
    // (b) the rest (misses, collisions, longer or non-ASCII words) go to a
    //     pending list that a per-lane state machine drains: lanes pull work
    //     from a block-wide LDS queue and advance one vocab probe per iteration,
    //     so no lane idles behind a long word.
    // (a) and (b) alternate in rounds so the pending list stays within
    // PEND_CAP: a round of (a) adds at most TOK_THREADS * TOK_UNROLL = PEND_CAP,
    // so it is admitted only while nothing is pending, and a chunk of more
    // pieces alternates between (a) and (b).
    lds_u16 *stage = (lds_u16 *)s_stage;
    // exceptions to "a piece has one id, in its first byte's slot" (wp_pack.hpp): the pending
    // walk sets the bit of every further id as it stages it (and clears them if the word ends
    // as [UNK]), the other paths set a finished piece's bits at once; the overrides were consumed barriers ago
    uint32_t *s_vx = reinterpret_cast<uint32_t *>(s_ovr);
    static_assert(4 * WP_VX_WORDS <= CHUNK && WP_VX_WORDS <= TOK_THREADS && WP_SLOTS == STAGE && WP_MAIN == CHUNK, "");
    if (tid < WP_VX_WORDS) s_vx[tid] = 0u;
    // Stop and fast-terminator bitmaps of the chunk's bytes and the first 16 of the right halo
    // (wp_extent.hpp), behind the exception bitmap: every lane writes the 16 bits of its own
    // bytes, lane 0 also those of bits CHUNK .. CHUNK + 15.  Words of S and F alternate, so
    // lane t's halves are u16 (t & 1) of u32 words 2 (t >> 1) and 2 (t >> 1) + 1.
    static_assert(4 * WP_VX_WORDS % 8 == 0 && 4 * WP_VX_WORDS + 8 * WX_WORDS <= CHUNK && WX_CHUNK == CHUNK &&
                      HALO_L + WX_BITS <= WIN,
                  "the bitmaps lie in s_ovr; their halo bits have bytes and record bits in the window");
    const lds_u64 *sf64 = (const lds_u64 *)(s_ovr + 4 * WP_VX_WORDS);
    {
        lds_u16 *sf16 = (lds_u16 *)(s_ovr + 4 * WP_VX_WORDS);
        lds_u32 *sf32 = (lds_u32 *)(s_ovr + 4 * WP_VX_WORDS);
        const WxStops own = wx_stops_from(sfm >> 16, sfm, rmask, wp_bits16(s_nabits, 16 * tid), nown);
        sf16[4 * (tid >> 1) + (tid & 1)] = (uint16_t)own.s;
        sf16[4 * (tid >> 1) + 2 + (tid & 1)] = (uint16_t)own.f;
        // the halo's 16 bytes, one a lane, by two ballots (no lane owns them, and a branch for
        // one lane would cost the wave a whole classification)
        const bool in16 = tid < WX_BITS - WX_CHUNK;
        const uint32_t hb16 = win[HALO_L + CHUNK + (tid & 15)];
        const uint32_t han = (uint32_t)__ballot(in16 && wx_is_alnum(hb16));
        const uint32_t htm = (uint32_t)__ballot(in16 && wx_is_term(hb16));
        const int64_t left = N - (c0 + CHUNK);
        const WxStops halo = wx_stops_from(han, htm, wp_bits16(rbits, HALO_L + CHUNK), 0u,
                                           left < 0 ? 0 : left < 16 ? (int)left : 16);
        if (tid == 0) {
            sf32[2 * (CHUNK / 32)] = halo.s;
            sf32[2 * (CHUNK / 32) + 1] = halo.f;
            sf32[2 * (CHUNK / 32) + 2] = 0u;
            sf32[2 * (CHUNK / 32) + 3] = 0u;
        }
    }
    auto stage_count = [&](int prel, int n) {
        if (n == 1) return;
        const WpRange r = wp_exception_range(prel, n);
        for (int wd = r.lo >> 5; wd <= (r.hi - 1) >> 5; ++wd) atomicOr(&s_vx[wd], wp_word_mask(wd, r.lo, r.hi));
    };
    if (tid == 0) {
        s_scratch[TOK_THREADS / 64 + 1] = 0;  // pending count
        s_scratch[TOK_THREADS / 64 + 2] = 0;  // deferred count
    }
    __syncthreads();
    PHASE_STAMP(10);
    const int lane = tid & 63;
    const lds_u32 *w32 = (const lds_u32 *)s_win;
    // word setup shared by (a) and (b): the word's length and fast flag from the two bitmaps
    // (both windows come with one read, next to the window's five dwords), its bytes
    // lower-cased by one OR -- inside the length every byte is an ASCII letter or digit --
    // or, CASED, as they are; returns false if the general path is needed
    auto word_setup = [&](int prel, W16 &lw, int &Lout) -> bool {
        const int wr = prel + HALO_L;
        const int a = wr >> 2;
        const uint32_t sh = (uint32_t)(wr & 3);
        const int q = prel + 1;
        const uint32_t x0 = w32[a], x1 = w32[a + 1], x2 = w32[a + 2], x3 = w32[a + 3], x4 = w32[a + 4];
        const uint64_t e0 = sf64[q >> 5], e1 = sf64[(q >> 5) + 1];  // {S, F} words
        const W16 raw{__builtin_amdgcn_alignbyte(x1, x0, sh), __builtin_amdgcn_alignbyte(x2, x1, sh),
                      __builtin_amdgcn_alignbyte(x3, x2, sh), __builtin_amdgcn_alignbyte(x4, x3, sh)};
        const WxExtent ex = wx_extent(wx_window((uint32_t)e0, (uint32_t)e1, q),
                                      wx_window((uint32_t)(e0 >> 32), (uint32_t)(e1 >> 32), q), raw.x);
        const WxMask m = CASED ? wx_keep(raw.x, raw.y, raw.z, raw.w, ex.len)
                               : wx_lower_keep(raw.x, raw.y, raw.z, raw.w, ex.len);
        lw = W16{m.x, m.y, m.z, m.w};
        Lout = ex.len;
        return ex.fast;
    };
    for (int r0 = 0; r0 < np;) {
    // (a) batched first probes
    for (; r0 < np && (int)s_scratch[TOK_THREADS / 64 + 1] <= PEND_CAP - TOK_THREADS * TOK_UNROLL;
         r0 += TOK_THREADS * TOK_UNROLL) {
        W16 cand[TOK_UNROLL];
        int prel_u[TOK_UNROLL];
        bool probe[TOK_UNROLL], pend[TOK_UNROLL];
#pragma unroll
        for (int u = 0; u < TOK_UNROLL; ++u) {
            const int pi = r0 + u * TOK_THREADS + tid;
            probe[u] = pend[u] = false;
            cand[u] = W16{0, 0, 0, 0};
            prel_u[u] = 0;
            if (pi >= np) continue;
            const uint32_t pc = s_pieces[pi];
            const int prel = (int)(pc & 0xFFFu);
            const uint32_t kind = pc >> 12;
            prel_u[u] = prel;
            if (kind == V_SPEC) {
                const int m = special_match(C, c0 + prel);
                stage[prel] = (uint16_t)T.special_id[m < 0 ? 0 : m];
            } else if (kind == V_ISO) {
                const uint32_t b = win[prel + HALO_L];
                if (b < 0x80u) {
                    stage[prel] = (uint16_t)T.ascii_id[b];
                } else if (!((s_nabits[CHUNK / 32 + (prel >> 5)] >> (prel & 31)) & 1u)) {
                    pend[u] = true;  // (else its id is in its stage slot: rare pass)
                }
            } else {
                W16 lw;
                int Lw;
                if (word_setup(prel, lw, Lw) && Lw <= F.maxlen) {
                    cand[u] = lw;
                    probe[u] = true;
                } else {
                    pend[u] = true;
                }
            }
        }
        FirstProbe pr[TOK_UNROLL];
#pragma unroll
        for (int u = 0; u < TOK_UNROLL; ++u) pr[u] = first_probe_load(F, cand[u]);
#pragma unroll
        for (int u = 0; u < TOK_UNROLL; ++u) {
            const int pi = r0 + u * TOK_THREADS + tid;
            if (probe[u]) {
                const int id = first_probe_result(pr[u], cand[u]);
                if (id >= 0) {
                    stage[prel_u[u]] = (uint16_t)id;
                } else {
                    pend[u] = true;
                }
            }
            const uint64_t pm = __ballot(pend[u]);
            if (pm) {
                const int leader = __builtin_ctzll(pm);
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(&s_scratch[TOK_THREADS / 64 + 1], (uint32_t)__popcll(pm));
                base = lane_bcast(base, leader);
                if (pend[u]) s_pend[base + __popcll(pm & ((1ull << lane) - 1ull))] = (uint16_t)pi;
            }
        }
        __syncthreads();  // the pending count is read by the loop test
    }
    PHASE_STAMP(11);
    int npend = (int)s_scratch[TOK_THREADS / 64 + 1];
    if (tid == 0) s_scratch[TOK_THREADS / 64 + 1] = 0;  // becomes the queue head
    __syncthreads();
    // (b) state machine over the pending pieces.  A pending word is worked by a group of G
    //     lanes (G = 64 / pending lanes, at most 8; wave-uniform): the group's lanes hold the same
    //     word state, lane g probes the candidates g * WP_NPROBE .. (g + 1) * WP_NPROBE - 1
    //     chars shorter than the longest remaining one, and the group takes the longest hit --
    //     the lowest lane with one -- so a step covers G * WP_NPROBE candidate lengths of
    //     WordPiece's longest-match-first walk instead of WP_NPROBE (a chunk holds ~12 pending
    //     words on held-out text, ~1 on the fixture: most lanes would otherwise idle).
    if (npend) {
        const int G = npend <= 8 ? 8 : npend > 32 ? 1 : 64 / npend;  // (lanes past the last group idle)
        const int gl = lane % G, g0 = lane - gl;    // lane in the group, the group's first lane
        const uint64_t gmask = ((1ull << G) - 1ull) << g0;
        const bool grouped = g0 + G <= 64;
        bool exhausted = !grouped;  // (a lane outside every group takes no word)
        bool active = false;  // a fast WordPiece state is live (the same in every lane of a group)
        int pi = 0, prel = 0, L = 0, start = 0, end = 0, nout = 0;
        W16 w{0, 0, 0, 0};
        for (;;) {
            const bool need = !active && !exhausted;
            const uint64_t nm = __ballot(need && gl == 0);
            if (nm) {
                const int leader = __builtin_ctzll(nm);
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(&s_scratch[TOK_THREADS / 64 + 1], (uint32_t)__popcll(nm));
                base = lane_bcast(base, leader);
                int q = (int)base + __popcll(nm & ((1ull << lane) - 1ull));  // (valid in the group's first lane)
                if (G > 1) q = __shfl(q, g0);
                if (need) {
                    if (q >= npend) {
                        exhausted = true;
                    } else {
                        pi = s_pend[q];
                        const uint32_t pc = s_pieces[pi];
                        prel = (int)(pc & 0xFFFu);
                        const uint32_t kind = pc >> 12;
                        const int64_t p = c0 + prel;
                        lds_u16 *out = stage + prel;
                        bool fits;
                        if (kind == V_OTHER && word_setup(prel, w, L)) {
                            fits = true;
                        } else {
                            fits = normalize_w16<CASED>(C, p, rec_end_of(C, rb_next, p),
                                                 kind == V_ISO, w, L);
                        }
                        if (fits) {
                            start = 0;
                            end = L < T.maxlen_first ? L : T.maxlen_first;
                            while (end < L && end > 0 && (w16_byte(w, end) & 0xC0u) == 0x80u) --end;
                            nout = 0;
                            active = end > 0;
                            if (!active && gl == 0) {  // no piece can match: the word is [UNK]
                                out[0] = (uint16_t)T.unk_id;
                            }
                        } else if (gl == 0) {
                            // deferred to (c) below: the cooperative lattice, or the general ISO char
                            const uint32_t d = atomicAdd(&s_scratch[TOK_THREADS / 64 + 2], 1u);
                            s_pend[d] = (uint16_t)pi;  // d < this round's consumed entries
                        }
                    }
                }
            }
            if (!__any(active || !exhausted)) break;
            if (active) {  // probe this lane's WP_NPROBE candidates, gl * WP_NPROBE chars below `end`
                const W16 sh = start ? shift_right_bytes(w, start) : w;
                const uint32_t cont = start > 0 ? 1u : 0u;
                int ek[WP_NPROBE];
                // (an ASCII word's chars are its bytes: no walk over continuation bytes)
                const bool ascii = ((w.x | w.y | w.z | w.w) & 0x80808080u) == 0u;
                int e0 = end;
                if (ascii) {
                    e0 = end - gl * WP_NPROBE > start ? end - gl * WP_NPROBE : start;
                } else {
                    for (int k = 0; k < gl * WP_NPROBE; ++k) e0 = e0 > start ? w16_prev_char(w, e0, start) : start;
                }
                ek[0] = e0;
#pragma unroll
                for (int k = 1; k < WP_NPROBE; ++k)
                    ek[k] = ek[k - 1] <= start ? start : ascii ? ek[k - 1] - 1 : w16_prev_char(w, ek[k - 1], start);
                W16 cw[WP_NPROBE];
                Probe Pk[WP_NPROBE];
#pragma unroll
                for (int k = 0; k < WP_NPROBE; ++k) {
                    const int nk = ek[k] - start;
                    cw[k] = keep_bytes(sh, nk);
                    Pk[k] = probe_load(T, hash16(cw[k], (uint32_t)nk, cont));
                }
                int id = -1, got = 0;
#pragma unroll
                for (int k = 0; k < WP_NPROBE; ++k) {
                    const int nk = ek[k] - start;
                    if (id < 0 && nk > 0) {
                        id = probe_result(Pk[k], (uint32_t)nk | (cont << 8), cw[k]);
                        got = nk;
                    }
                }
                int e1 = ek[WP_NPROBE - 1];
                if (G > 1) {  // the group's longest hit: its lowest lane with one
                    const uint64_t hm = __ballot(id >= 0) & gmask;
                    const int src = hm ? __builtin_ctzll(hm) : g0;
                    id = __shfl(id, src);
                    got = __shfl(got, src);
                    e1 = __shfl(e1, g0 + G - 1);
                }
                const int n1 = e1 - start;
                lds_u16 *out = stage + prel;
                if (id >= 0) {
                    if (gl == 0) {
                        out[nout] = (uint16_t)id;
                        if (nout) atomicOr(&s_vx[(prel + nout) >> 5], 1u << ((prel + nout) & 31));  // a further id
                    }
                    ++nout;
                    start += got;
                    if (start >= L) {
                        active = false;
                    } else {
                        end = L < start + T.maxlen_cont ? L : start + T.maxlen_cont;
                        while (end < L && end > start && (w16_byte(w, end) & 0xC0u) == 0x80u) --end;
                    }
                } else {
                    end = n1 > 0 ? w16_prev_char(w, e1, start) : start;
                    if (end <= start) {  // no piece matches here: the whole word is [UNK]
                        if (gl == 0) {
                            out[0] = (uint16_t)T.unk_id;
                            for (int wd = (prel + 1) >> 5; nout > 1 && wd <= (prel + nout - 1) >> 5; ++wd)
                                atomicAnd(&s_vx[wd], ~wp_word_mask(wd, prel + 1, prel + nout));  // its staged ids
                        }
                        active = false;
                    }
                }
            }
        }
        // (c) deferred words (normalization longer than 16 bytes, DEL runs,
        //     canonical ordering): one at a time, normalized by lane 0 into LDS
        //     (the pending list's space, free now: PEND_CAP u16 hold the
        //     MAX_WORD_BYTES of the longest word), then the WordPiece lattice:
        //     every (start, length) candidate with a vocab piece of that length
        //     is one probe task dealt across the wave, and each start keeps its
        //     longest hit (atomic max of length << 16 | id); lane 0 walks
        //     greedy longest-match-first over them.  Probe latencies per word
        //     ~ candidates / 64, where probing one candidate at a time pays one
        //     per candidate.  An ISO char whose normalization is longer than 16
        //     bytes comes here too: lane 0 probes it one candidate at a time.
        static_assert(MAX_WORD_BYTES <= 2 * PEND_CAP && LW_BUF + 4 * LW_MAX <= 2 * PEND_CAP, "s_pend holds the word");
        __syncthreads();
        const int ndef = (int)s_scratch[TOK_THREADS / 64 + 2];
        if (ndef) {
            uint32_t dl[PEND_CAP / 64];
#pragma unroll
            for (int j = 0; j < PEND_CAP / 64; ++j) {
                const int d = 64 * j + lane;
                dl[j] = d < ndef ? s_pend[d] : 0u;
            }
            __syncthreads();
            lds_u8 *wb = (lds_u8 *)s_pend;
            const lds_u32 *wb32 = (const lds_u32 *)s_pend;
            lds_u32 *best = (lds_u32 *)s_pend + LW_BUF / 4;
            for (int d = 0; d < ndef; ++d) {
                uint32_t mine = dl[0];
#pragma unroll
                for (int j = 1; j < PEND_CAP / 64; ++j)
                    if ((d >> 6) == j) mine = dl[j];
                const int dpi = lane_bcast((int)mine, d & 63);
                const int dprel = (int)(s_pieces[dpi] & 0xFFFu);
                const int64_t dp = c0 + dprel;
                lds_u16 *dout = stage + dprel;
                int dL = 0;
                if (lane == 0 && (s_pieces[dpi] >> 12) == V_ISO) {
                    int len;
                    const uint32_t e = uentry(T, decode(C, dp, win[dprel + HALO_L], &len));
                    const int nb = append_norm(C, e, dp, len, wb, 0);
                    stage_count(dprel, wordpiece_general(T, wb, nb, dout));
                } else if (lane == 0) {
                    const int64_t rend = rec_end_of(C, rb_next, dp);
                    int nch, nby;
                    const int64_t iend = word_extent(C, dp, rend, &nch, &nby);
                    if (nch > MAX_WORD_CHARS) {
                        dout[0] = (uint16_t)T.unk_id;
                    } else if (nby > LW_MAX || T.wp_long_pieces) {
                        stage_count(dprel, word_general<CASED>(C, dp, iend, wb, dout));
                    } else {
                        dL = word_materialize<CASED>(C, dp, iend, wb);
                        for (int k = dL; k < dL + 20; ++k) wb[k] = 0;
                    }
                }
                dL = lane_bcast(dL, 0);
                if (dL == 0) continue;  // wave-uniform
                for (int k = lane; k < dL; k += 64) best[k] = 0u;
                __syncthreads();
                const int nf = T.wp_nlens[0], nc = T.wp_nlens[1];
                const int ntask = nf + (dL - 1) * nc;
                for (int k = lane; k < ntask; k += 64) {
                    int st, n;
                    if (k < nf) {
                        st = 0;
                        n = T.wp_lens[k];
                    } else {
                        st = 1 + (k - nf) / nc;
                        n = T.wp_lens[LW_MAX + (k - nf) % nc];
                    }
                    if (st + n > dL || (wb[st] & 0xC0u) == 0x80u || (st + n < dL && (wb[st + n] & 0xC0u) == 0x80u))
                        continue;
                    const uint32_t cont = st > 0 ? 1u : 0u;
                    uint32_t h = hinit((uint32_t)n, cont);
                    for (int b0 = 0; b0 < n; b0 += 16) {
                        const W16 blk = lds_w16(wb32, st + b0, n - b0);
                        h = hmix(hmix(hmix(hmix(h, blk.x), blk.y), blk.z), blk.w);
                    }
                    h = hfinal(h);
                    const W16 first = lds_w16(wb32, st, n);
                    const Probe P = probe_load(T, h);
                    const uint32_t key = (uint32_t)n | (cont << 8);
                    int id = -1;
                    for (int which = 0; which < 2 && id < 0; ++which) {
                        const uint4 a = which ? P.a2 : P.a1, b = which ? P.b2 : P.b1;
                        if (!slot_match(a, b, key, first)) continue;
                        bool ok = true;
                        for (int x = 16; x < n && ok; ++x) ok = T.vpool[a.z + x] == wb[st + x];
                        if (ok) id = (int32_t)a.y;
                    }
                    if (id >= 0)
                        __hip_atomic_fetch_max(best + st, ((uint32_t)n << 16) | (uint32_t)id, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                __syncthreads();
                if (lane == 0) {
                    int nout = 0;
                    for (int st = 0; st < dL;) {
                        const uint32_t bv = best[st];
                        if (!bv) {
                            nout = -1;
                            break;
                        }
                        dout[nout++] = (uint16_t)(bv & 0xFFFFu);
                        st += (int)(bv >> 16);
                    }
                    if (nout < 0) {
                        dout[0] = (uint16_t)T.unk_id;
                        nout = 1;
                    }
                    stage_count(dprel, nout);
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        s_scratch[TOK_THREADS / 64 + 1] = 0;  // the next round's pending count
        s_scratch[TOK_THREADS / 64 + 2] = 0;  // ... and deferred count
    }
    __syncthreads();
    }
    PHASE_STAMP(7);

    // ---- 5. compact ids into this chunk's tokc slice ------------------------------
    // Lane t owns the stage slots [16t, 16t + 16) -- lanes 0-7 also the tail slots
    // [CHUNK + 16t, ...), which only the chunk's last word reaches.  A slot holds an id where a
    // piece starts (pmask, still in registers) or the exception bitmap says otherwise
    // (wp_pack.hpp); a slot's list position is a wave sum plus a popcount, and the record
    // boundaries' offsets come from the same sums in every case below.  (a) A chunk without an
    // exception bit is gathered through the piece list; (b) one with exceptions is packed slot
    // by slot in LDS (pack16) and copied out; (c) one with exceptions and more ids than the
    // window holds stores straight to its slice.
    const uint32_t vx16 = wp_bits16(s_vx, 16 * tid);
    const uint32_t vmain = pmask ^ vx16;
    const uint32_t vtail = tid < WP_TAIL_LANES ? wp_bits16(s_vx, CHUNK + 16 * tid) : 0u;
    uint32_t tot2;
    const uint32_t ex2 = block_excl_sum<TOK_THREADS>(wp_lane_counts(vmain, vtail), &tot2, s_scratch);
    const uint32_t total = wp_total(tot2);
    const uint32_t base = wp_main_base(ex2);
    uint16_t *dst = tokc + ci * STAGE;  // (a slice is STAGE u16 = 2304 B: 16-B aligned)
    // The list is first packed in LDS (the text window is dead now) so the wave
    // writes it as whole 16-B lanes: scattered 4-B stores cost 3.5x the list's
    // bytes in HBM writes (PMC WRITE_SIZE 851 MB vs 240 MB).  It is stored as it
    // lies there, u16 (every id is below 65,536), 8 ids a lane; the last store's
    // slots past `total` hold whatever the window held.  Plain stores, not
    // non-temporal ones: the rows kernel reads the lists next and is bound by the
    // latency of those loads, so the lists (0.1 GB a 256 MiB arena) should still
    // be in the memory-side cache then (mlm rows 0.324 ms after non-temporal
    // stores, 0.270 after plain ones; the tokenizer itself 1.118 -> 1.116 ms;
    // profiles/r07/lists).
    // A further id adds to `total` and a piece without an id takes from it, so a chunk whose total
    // differs from its piece count has exceptions: one scalar compare sends it on, and only a
    // chunk with total == np pays the wave vote over the bitmap.
    if (total == (uint32_t)np && !__any((vx16 | vtail) != 0u)) {
        // (a) no exception bit in the chunk: every piece has exactly one id, in the stage slot
        // of its first byte, so list entry e is s_stage[s_pieces[e] & 0xFFF] and total == np.
        // The lane of entries [8k, 8k + 8) reads their descriptors with one 16-B read, their
        // ids from the slots the descriptors name, and stores 16 bytes to the slice.  An entry
        // at or past np holds a stale descriptor: wp_pair_slots keeps its slot inside the stage,
        // and what the last store leaves past `total` is unspecified, as below.  A chunk of more
        // ids than the window holds comes here too.
        for (uint32_t e = 8u * (uint32_t)tid; e < total; e += 8u * TOK_THREADS) {
            const uint4 d = *reinterpret_cast<const uint4 *>(s_pieces + e);
            const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t s2 = wp_pair_slots(dw[j]);  // (entries past np: stale, kept inside the stage)
                o[j] = (uint32_t)s_stage[s2 & 0xFFFFu] | ((uint32_t)s_stage[s2 >> 16] << 16);
            }
            u32x4 v;
            v.x = o[0];
            v.y = o[1];
            v.z = o[2];
            v.w = o[3];
            *reinterpret_cast<u32x4 *>(dst + e) = v;
        }
    } else if (total <= (uint32_t)(WIN / 2)) {
        lds_u16 *packed = (lds_u16 *)s_win;
        // 16 unconditional 2-B stores a lane, no loop and no branch: a slot without an id goes
        // to a per-lane dump slot in the pending list's space (dead now)
        lds_u16 *dump = (lds_u16 *)s_pend + tid;
        auto pack16 = [&](const uint16_t *slots, uint32_t valid, uint32_t b0) {
            const uint4 a = *reinterpret_cast<const uint4 *>(slots), b = *reinterpret_cast<const uint4 *>(slots + 8);
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                lds_u16 *to = (valid >> i) & 1u ? packed + wp_pos(b0, valid, i) : dump;
                *to = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
            }
        };
        pack16(s_stage + 16 * tid, vmain, base);
        if (tot2 >> 16) {  // block-uniform
            if (tid < WP_TAIL_LANES) pack16(s_stage + CHUNK + 16 * tid, vtail, wp_tail_base(ex2, tot2));
        }
        __syncthreads();
        const lds_u32 *p32 = (const lds_u32 *)s_win;
        for (uint32_t e = 8u * (uint32_t)tid; e < total; e += 8u * TOK_THREADS) {
            u32x4 v;
            v.x = p32[e >> 1];
            v.y = p32[(e >> 1) + 1];
            v.z = p32[(e >> 1) + 2];
            v.w = p32[(e >> 1) + 3];
            *reinterpret_cast<u32x4 *>(dst + e) = v;
        }
    } else {  // more ids than the window holds (runs of punctuation): straight to the slice
        uint32_t b0 = base;
        for (uint32_t m = vmain; m; m &= m - 1) dst[b0++] = s_stage[16 * tid + __builtin_ctz(m)];
        b0 = wp_tail_base(ex2, tot2);
        for (uint32_t m = vtail; m; m &= m - 1) dst[b0++] = s_stage[CHUNK + 16 * tid + __builtin_ctz(m)];
    }
    PHASE_STAMP(8);
    if (tid == 0) chunk_cnt[ci] = total;
    // record boundaries owned by this chunk: ids of the chunk before the boundary, from the
    // base and the valid mask of the lane that owns the boundary's byte.  The loop is
    // wave-uniform (every lane serves the shuffles).
    const int k_lo = (int)(r_lo - ra);
    for (int k0 = k_lo; k0 < nrb; k0 += TOK_THREADS) {
        const int k = k0 + tid;
        const int64_t pos = k < nrb ? (int64_t)off[ra + k] : c1;
        const bool own = pos >= c0 && pos < c1;
        const int rel = own ? (int)(pos - c0) : 0;
        const uint32_t lb = (uint32_t)__shfl((int)base, wp_boundary_lane(rel));
        const uint32_t lv = (uint32_t)__shfl((int)vmain, wp_boundary_lane(rel));
        if (own) rec_local[ra + k] = wp_boundary_offset(lb, lv, rel);
        if (!__any(own)) break;  // (offsets ascend)
    }
    PHASE_STAMP(9);
}

#ifdef SDL_STAMPS
void print_phase_cycles() {
    unsigned long long h[16];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(sdl_phase_cycles), sizeof(h)) != hipSuccess) return;
    static const char *names[] = {"", "load+classify+rbits", "opener-list", "openers", "fill+lookback",
                                  "scan+pieces", "-", "wp-pending", "compact", "rec_local", "wp-init",
                                  "wp-first-probes", "rare-leads"};
    unsigned long long tot = 0;
    for (int k = 1; k <= 12; ++k) tot += h[k];
    fprintf(stderr, "[stamps] block-cycles by phase (wave 0, all blocks, all calls):");
    for (int k = 1; k <= 12; ++k)
        if (k != 6) fprintf(stderr, " %s=%.1f%%", names[k], 100.0 * h[k] / (tot ? tot : 1));
    fprintf(stderr, " total=%llu\n", tot);
}
#endif

hipError_t launch_wordpiece_chunks(const DevTok &T, const DevFirst &F, bool cased, const uint8_t *text, int64_t N,
                                   const uint64_t *off, int64_t R, uint32_t *ranges, uint16_t *tokc, uint32_t *chunk_cnt, uint32_t *rec_local,
                                   hipStream_t st, int64_t c_begin, int64_t c_end) {
    const int64_t n_chunks = (N + CHUNK - 1) / CHUNK;
    if (c_end < 0 || c_end > n_chunks) c_end = n_chunks;
    if (c_begin < 0) c_begin = 0;
    if (c_end <= c_begin) return hipSuccess;
    const dim3 grid((unsigned)(c_end - c_begin)), block(TOK_THREADS);
    if (cased)
        hipLaunchKernelGGL(k_wordpiece_chunks<true>, grid, block, 0, st, T, F, text, N, off, R, ranges, tokc, chunk_cnt,
                           rec_local, c_begin);
    else
        hipLaunchKernelGGL(k_wordpiece_chunks<false>, grid, block, 0, st, T, F, text, N, off, R, ranges, tokc, chunk_cnt,
                           rec_local, c_begin);
    return hipGetLastError();
}

}  // namespace sdl
