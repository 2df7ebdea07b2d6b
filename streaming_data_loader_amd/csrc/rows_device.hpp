// Device code shared by the rows kernels (pipeline.hip) and the fused tiny-push tail of the
// WordPiece chunk kernel (tokenize_wordpiece.hip): chunk-list compaction, per-record framing,
// the Philox mask contract and one row's planes.  A row's ids come from the dense array the
// compaction makes, or (WordPiece, large calls: row_one<.., LISTS>) straight from the packed u16
// chunk lists the tokenizer wrote, indexed as list_index.hpp says.
#pragma once
#include "common.hpp"
#include "device_util.hpp"
#include "kernels.hpp"
#include "list_index.hpp"
#include "mlm_pick.hpp"

namespace sdl {

static_assert(LIST_CHUNK == CHUNK && LIST_STRIDE == STAGE, "list_index.hpp restates the chunk geometry");

constexpr int COMPACT_CPW = 4;  // chunks per wave: their loads are in flight together
// one wave: chunks [cb, cb + COMPACT_CPW).  PART 1: only when the call has no long items, 2: only
// when it has (separate kernels keep the plain copy's registers), 0: either.
// E16: the lists are packed u16 (WordPiece: stride u16 slots a chunk, no long items).
template <int PART = 0, bool E16 = false>
__device__ __forceinline__ void compact_wave(int64_t cb, const uint32_t *__restrict__ tokc,
                                             const uint32_t *__restrict__ chunk_cnt,
                                             const uint32_t *__restrict__ chunk_off, int64_t n_chunks,
                                             uint32_t *__restrict__ tok, const uint32_t *long_count,
                                             const uint32_t *__restrict__ chunk_ent,
                                             const BpeLong *__restrict__ long_list,
                                             const uint16_t *__restrict__ long_scratch,
                                             const uint32_t *__restrict__ long_pool, int64_t stride) {
    const int lane = threadIdx.x & 63;
    uint32_t n[COMPACT_CPW], o[COMPACT_CPW];
#pragma unroll
    for (int j = 0; j < COMPACT_CPW; ++j) {
        const bool in = cb + j < n_chunks;
        n[j] = in ? chunk_cnt[cb + j] : 0u;
        o[j] = in ? chunk_off[cb + j] : 0u;
    }
    // (unigram: Viterbi job markers are in every call's lists)
    const bool has_long = !E16 && long_count && (long_pool != nullptr || *long_count != 0);
    if ((PART == 1 && has_long) || (PART == 2 && !has_long)) return;
    // entry i of chunk c's list
    auto entry = [&](int64_t c, uint32_t i) -> uint32_t {
        if constexpr (E16)
            return __builtin_nontemporal_load(reinterpret_cast<const uint16_t *>(tokc) + c * stride + i);
        else
            return __builtin_nontemporal_load(tokc + c * stride + i);
    };
    if (!has_long) {
        // lane-contiguous dwords: every store instruction writes 256 B of the
        // dense array back to back (at any alignment); the first 256 ids of all
        // the wave's chunks are loaded before any is stored
        uint32_t v[COMPACT_CPW][4];
#pragma unroll
        for (int j = 0; j < COMPACT_CPW; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = 64 * k + lane;
                v[j][k] = i < n[j] ? entry(cb + j, i) : 0u;
            }
#pragma unroll
        for (int j = 0; j < COMPACT_CPW; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t i = 64 * k + lane;
                if (i < n[j]) tok[(uint64_t)o[j] + i] = v[j][k];
            }
        for (int j = 0; j < COMPACT_CPW; ++j) {  // chunks with more than 256 ids
            for (uint32_t i0 = 256; i0 < n[j]; i0 += 256) {
                uint32_t w[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t i = i0 + 64 * k + lane;
                    w[k] = i < n[j] ? entry(cb + j, i) : 0u;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t i = i0 + 64 * k + lane;
                    if (i < n[j]) tok[(uint64_t)o[j] + i] = w[k];
                }
            }
        }
        return;
    }
    if constexpr (E16) return;
    // byte-level BPE / unigram with long items: an entry LONG_MARK | i stands
    // for the k ids of long piece i (in long_scratch at its byte position) or
    // of pool item i; a unigram Viterbi job's entry LONG_MARK | UNI_JOB_BIT |
    // k << 24 | pos for the k u16 ids at pos of its chunk's results region.
    // The wave's chunks go in lockstep, 64 entries of each a step, so their
    // dependent loads (entry -> item -> ids) are in flight together.
    uint32_t ne[COMPACT_CPW], written[COMPACT_CPW], nemax = 0;
#pragma unroll
    for (int j = 0; j < COMPACT_CPW; ++j) {
        ne[j] = cb + j < n_chunks ? chunk_ent[cb + j] : 0u;  // entries written by the chunk kernel
        written[j] = 0;
        nemax = ne[j] > nemax ? ne[j] : nemax;
    }
    for (uint32_t e0 = 0; e0 < nemax; e0 += 64) {
        const uint32_t e = e0 + lane;
        uint32_t x[COMPACT_CPW], w[COMPACT_CPW];
#pragma unroll
        for (int j = 0; j < COMPACT_CPW; ++j)
            x[j] = e < ne[j] ? __builtin_nontemporal_load(tokc + (cb + j) * stride + e) : 0u;
#pragma unroll
        for (int j = 0; j < COMPACT_CPW; ++j) {
            const bool mark = (x[j] & 0x80000000u) != 0u;
            const bool job = long_pool && (x[j] & UNI_JOB_BIT);
            w[j] = e >= ne[j] ? 0u : !mark ? 1u : job ? (x[j] >> 24) & 63u : long_pool ? long_pool[x[j] & 0x7FFFFFFFu]
                                                                                    : long_list[x[j] & 0x7FFFFFFFu].k;
        }
#pragma unroll
        for (int j = 0; j < COMPACT_CPW; ++j) {
            const uint32_t incl = wave_incl_sum(w[j]);
            const uint32_t at = written[j] + incl - w[j];
            uint32_t *dst = tok + o[j];
            if (e < ne[j] && at < n[j]) {
                if (!(x[j] & 0x80000000u)) {
                    dst[at] = x[j];
                } else if (long_pool && (x[j] & UNI_JOB_BIT)) {  // unigram Viterbi job
                    const uint16_t *jr = reinterpret_cast<const uint16_t *>(tokc + (cb + j) * stride + UNI_JR_OFF) +
                                         (x[j] & 0xFFFu);
                    for (uint32_t q0 = 0; q0 < w[j]; q0 += 8) {  // (8 loads in flight, then 8 stores)
                        uint32_t id[8];
#pragma unroll
                        for (uint32_t r = 0; r < 8; ++r) id[r] = q0 + r < w[j] ? jr[q0 + r] : 0u;
#pragma unroll
                        for (uint32_t r = 0; r < 8; ++r)
                            if (q0 + r < w[j]) dst[at + q0 + r] = id[r];
                    }
                } else if (long_pool) {  // unigram long item: [k, ids...] in the pool
                    const uint32_t po = x[j] & 0x7FFFFFFFu;
                    for (uint32_t q = 0; q < w[j]; ++q) dst[at + q] = long_pool[po + 1 + q];
                } else {
                    const uint64_t pos = long_list[x[j] & 0x7FFFFFFFu].pos;
                    for (uint32_t q = 0; q < w[j]; ++q) dst[at + q] = long_scratch[pos + q];
                }
            }
            written[j] += (uint32_t)lane_bcast((int)incl, 63);
        }
    }
}

// a small call's chunks [cb, cb + COMPACT_CPW) into its dense array: u16 lists (WordPiece) or u32 entries
__device__ __forceinline__ void compact_small(const SmallDown &d, int64_t cb, const uint32_t *__restrict__ chunk_off,
                                              int64_t n_chunks) {
    if (d.list16)
        compact_wave<0, true>(cb, d.tokc, d.chunk_cnt, chunk_off, n_chunks, d.tok, nullptr, nullptr, nullptr, nullptr,
                              nullptr, d.stride);
    else
        compact_wave(cb, d.tokc, d.chunk_cnt, chunk_off, n_chunks, d.tok, d.long_count, d.chunk_ent, d.long_list,
                     d.long_scratch, d.long_pool, d.stride);
}

// ---------------------------------------------------------------------------
// Per record: where its ids start, how many, and how many rows it yields.
// ---------------------------------------------------------------------------
// (returns the record's rows)
__device__ __forceinline__ uint32_t record_one(const RowParams &P, const uint64_t *__restrict__ off, int64_t r, int64_t N,
                                               const uint32_t *__restrict__ chunk_off, int64_t n_chunks,
                                               const uint32_t *__restrict__ rec_local, uint32_t *__restrict__ rec_tok,
                                               uint32_t *__restrict__ rec_cnt, uint32_t *__restrict__ rec_rows) {
    auto tok_off = [&](int64_t q) -> uint32_t {
        const int64_t p = (int64_t)off[q];
        // (chunk_off[n_chunks], the total, is final once the last segment is scanned:
        // only the last segment holds records that end at N)
        return p >= N ? chunk_off[n_chunks] : chunk_off[p / CHUNK] + rec_local[q];
    };
    const uint32_t a = tok_off(r), b = tok_off(r + 1);
    const uint32_t cnt = b - a;
    const uint32_t n = cnt + (uint32_t)(P.n_pre + P.n_post);  // encode_mask framing
    uint32_t rows = 0;
    if (n >= (uint32_t)P.min_ids) rows = P.chunk ? ceil_div_u32(n, (uint32_t)P.S) : 1u;  // gen_batcher.rs:74-80
    rec_tok[r] = a;
    rec_cnt[r] = cnt;
    rec_rows[r] = rows;
    return rows;
}

// ---------------------------------------------------------------------------
// RNG contract: Philox4x32-10 (Salmon et al., SC'11), as oracle/sdl_oracle.c.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

__device__ __forceinline__ uint32_t mlm_key(uint64_t seed, uint64_t rec, uint32_t chunk, uint32_t pos) {
    const uint4 c = philox4x32_10(make_uint4(pos >> 2, chunk, (uint32_t)rec, (uint32_t)(rec >> 32)), (uint32_t)seed,
                                  (uint32_t)(seed >> 32));
    const uint32_t s = pos & 3u;
    return s == 0 ? c.x : s == 1 ? c.y : s == 2 ? c.z : c.w;
}

// framing id k (< MAX_FRAME) without dynamic indexing of the kernel argument
__device__ __forceinline__ int32_t frame_id(const int32_t (&a)[MAX_FRAME], int k) {
    return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3];
}

// Row layout of k_rows: lane L owns positions 256*m + 4*L + w (w = 0..3), so
// one Philox block (4 words) is exactly one lane's keys for round m and every
// plane store is one 16-byte write per lane.
//
// Marks the k smallest (key, position) pairs of a row held as key[m][w]: a
// radix select of the k-th smallest key with wave ballots, then a
// position-ordered tie-break among keys equal to it.  The descent stops as soon
// as exactly k keys lie below the candidate (after ~log2(S) + 2 of the 32
// steps for distinct keys), which selects the same set.
template <int MR>
__device__ __forceinline__ void select_k_smallest(const uint32_t (&key)[MR][4], int k, bool (&sel)[MR][4]) {
    if (k <= 0) {
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) sel[m][w] = false;
        return;
    }
    uint32_t prefix = 0;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = prefix | (1u << bit);
        int c = 0;
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) c += __popcll(__ballot(key[m][w] < cand));
        if (c == k) {  // exactly the k smallest keys lie below cand: no tie to break
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int w = 0; w < 4; ++w) sel[m][w] = key[m][w] < cand;
            return;
        }
        if (c < k) prefix = cand;
    }
    int c_lt = 0;
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) c_lt += __popcll(__ballot(key[m][w] < prefix));
    const int need = k - c_lt;
    const uint64_t lt_mask = (1ull << lane_id()) - 1ull;
    int before = 0;  // equal keys in earlier rounds
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        uint64_t eq[4];
        int lower = 0;  // equal keys of this round in lower lanes
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            eq[w] = __ballot(key[m][w] == prefix);
            lower += __popcll(eq[w] & lt_mask);
        }
        int own = 0;  // equal keys of this lane at lower w
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const bool e = key[m][w] == prefix;
            sel[m][w] = key[m][w] < prefix || (e && before + lower + own < need);
            own += e ? 1 : 0;
        }
#pragma unroll
        for (int w = 0; w < 4; ++w) before += __popcll(eq[w]);
    }
}

// The same selection, usually in far fewer steps: the Philox keys are uniform,
// so an interpolation search over the key range (the next threshold guessed
// from the counts at the bracket's ends) lands on a threshold with exactly k
// keys below it in ~3-4 counts instead of the radix descent's ~log2(S) + 2.
// Any threshold with exactly k keys below it marks the same k-smallest set; a
// tie at the k-th key (no such threshold) or a slow bracket falls back to the
// radix select.
constexpr int ROWS_INTERP_STEPS = 8;
template <int MR>
__device__ __forceinline__ void select_k_smallest_interp(const uint32_t (&key)[MR][4], int k, int nvalid,
                                                         bool (&sel)[MR][4]) {
    if (k > 0 && k < nvalid) {
        uint32_t lo = 0, hi = 0xFFFFFFFFu;  // count(key < lo) = c_lo < k < c_hi ~ count(key < hi)
        int c_lo = 0, c_hi = nvalid;
#pragma unroll 1
        for (int it = 0; it < ROWS_INTERP_STEPS && hi - lo > 1u; ++it) {
            const float f = ((float)(k - c_lo) + 0.5f) / (float)(c_hi - c_lo);
            uint32_t cand = lo + (uint32_t)((float)(hi - lo) * f);
            cand = cand <= lo ? lo + 1u : cand >= hi ? hi - 1u : cand;
            cand = __builtin_amdgcn_readfirstlane(cand);
            int c = 0;
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int w = 0; w < 4; ++w) c += __popcll(__ballot(key[m][w] < cand));
            if (c == k) {
#pragma unroll
                for (int m = 0; m < MR; ++m)
#pragma unroll
                    for (int w = 0; w < 4; ++w) sel[m][w] = key[m][w] < cand;
                return;
            }
            if (c < k) {
                lo = cand;
                c_lo = c;
            } else {
                hi = cand;
                c_hi = c;
            }
        }
    }
    select_k_smallest<MR>(key, k, sel);
}

__device__ __forceinline__ void store4(int32_t *p, int j0, int S, bool vec, int32_t a, int32_t b, int32_t c,
                                       int32_t d) {
    if (vec) {  // the planes stream out: non-temporal, they are not re-read by this pass
        typedef int32_t v4i __attribute__((ext_vector_type(4)));
        if (j0 < S) __builtin_nontemporal_store(v4i{a, b, c, d}, reinterpret_cast<v4i *>(p + j0));
    } else {
        if (j0 < S) p[j0] = a;
        if (j0 + 1 < S) p[j0 + 1] = b;
        if (j0 + 2 < S) p[j0 + 2] = c;
        if (j0 + 3 < S) p[j0 + 3] = d;
    }
}

// The framed ids of a row's positions: id[m][w] is position 256 m + 4 lane + w of the row that
// starts at framed index `base` of its record (cnt ids from t0 on) and fills l positions; 0 past
// them.  LISTS: c / bnd / nl are the row's first chunk, the boundaries loaded from it on and the
// chunks scanned (row_one).
template <int MR>
struct RowIds {
    int32_t v[MR][4];
};
template <int MR, bool LISTS>
__device__ __forceinline__ RowIds<MR> row_ids(const RowParams &P, const TokSrc &src, uint32_t c, uint32_t bnd,
                                              int64_t nl, uint32_t t0, uint32_t cnt, int64_t base, int l, int lane) {
    int32_t id[MR][4];
    if constexpr (LISTS) {
        // the row's ids are [rel0, rel1) of the record's, [t_first, t_last] of the call's, and lie
        // at its positions [jlo, jhi); before them the opening frame, after them the closing one
        const int64_t rel0 = base > P.n_pre ? base - P.n_pre : 0;
        const int64_t rel1 = base + l - P.n_pre < (int64_t)cnt ? base + l - P.n_pre : (int64_t)cnt;
        const int jlo = (int)(rel0 + P.n_pre - base), jhi = (int)(rel1 + P.n_pre - base);
        // id index of position 256 m + 4 lane (+ w); a framing position's is never used
        const uint32_t tb = t0 + (uint32_t)(base - P.n_pre) + 4u * (uint32_t)lane;
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) id[m][w] = 0;
        if (rel0 < rel1) {  // (wave-uniform, as everything derived from g alone)
            const uint32_t t_last = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t0 + (uint32_t)rel1 - 1u));
            const uint16_t *__restrict__ lc = src.lists + (int64_t)c * STAGE;
            if ((uint32_t)__builtin_amdgcn_readlane((int)bnd, 63) > t_last) {
                uint32_t q[MR][4];  // boundaries at or below the id: its chunk is c + q
#pragma unroll
                for (int m = 0; m < MR; ++m)
#pragma unroll
                    for (int w = 0; w < 4; ++w) q[m][w] = 0;
#pragma unroll 1
                for (int b = 1; b < 64; ++b) {
                    const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)bnd, b);
                    if (x > t_last) break;
#pragma unroll
                    for (int m = 0; m < MR; ++m)
#pragma unroll
                        for (int w = 0; w < 4; ++w) q[m][w] += tb + 256u * m + w >= x ? 1u : 0u;
                }
#pragma unroll
                for (int m = 0; m < MR; ++m)
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const int j = 256 * m + 4 * lane + w;
                        const uint32_t lo = (uint32_t)__shfl((int)bnd, (int)(q[m][w] & 63u));
                        const uint32_t e = q[m][w] * (uint32_t)STAGE + (tb + 256u * m + w - lo);
                        if (j >= jlo && j < jhi) id[m][w] = (int32_t)lc[e];
                    }
            } else {
                // (one position of every lane a step; the selects keep id in registers)
#pragma unroll 1
                for (int i = 0; i < 4 * MR; ++i) {
                    const int j = 256 * (i >> 2) + 4 * lane + (i & 3);
                    const bool is_id = j >= jlo && j < jhi;
                    int32_t v = 0;
                    if (is_id) {
                        const uint32_t t = tb + 256u * (uint32_t)(i >> 2) + (uint32_t)(i & 3);
                        const int64_t cc = list_chunk_of(src.chunk_off, (int64_t)c, nl - 1, t);
                        v = (int32_t)src.lists[list_slot(src.chunk_off, cc, t)];
                    }
#pragma unroll
                    for (int m = 0; m < MR; ++m)
#pragma unroll
                        for (int w = 0; w < 4; ++w) id[m][w] = i == 4 * m + w && is_id ? v : id[m][w];
                }
            }
        }
        const int post0 = (int)(base - P.n_pre - (int64_t)cnt);  // (+ j: the closing frame's index)
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int j = 256 * m + 4 * lane + w;
                if (j < l && j < jlo) id[m][w] = frame_id(P.pre, (int)base + j);
                if (j < l && j >= jhi) id[m][w] = frame_id(P.post, post0 + j);
            }
    } else {
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int j = 256 * m + 4 * lane + w;
            int32_t v = 0;
            if (j < l) {
                const int64_t f = base + j;
                if (f < P.n_pre) v = frame_id(P.pre, (int)f);
                else if (f < P.n_pre + (int64_t)cnt) v = (int32_t)src.tok[t0 + (f - P.n_pre)];
                else v = frame_id(P.post, (int)(f - P.n_pre - cnt));
            }
            id[m][w] = v;
        }
    }
    RowIds<MR> out;
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) out.v[m][w] = id[m][w];
    return out;
}

// One row g of the call (a wave): BertData::put_data (+ mask_batch) / GptData::put_data framing and
// planes; g >= G: a padding row of the last batch.  late_bits: the row's mask words (LATE).
//
// LISTS: the ids are read from the WordPiece chunk lists themselves (TokSrc, list_index.hpp), not
// from a dense copy.  The row's first id lies in chunk c = row_chunk[g] (k_row_map).  One
// coalesced load gives lane b the boundary chunk_off[c + b]; a row normally ends 3-4 chunks on, so
// every id's chunk is a count of the few boundaries at or below its index (wave-uniform walk over
// them) and its list's start a cross-lane read of the loaded boundaries: no dependent global load
// between the boundaries and the ids.  A row that runs past the 63 loaded boundaries (a long run
// of chunks without ids) searches chunk_off per lane instead -- any span.
template <int MR, bool RM1, bool LATE, bool LISTS = false>
__device__ __forceinline__ void row_one(const RowParams &P, const TokSrc &src,
                                        const uint32_t *__restrict__ rec_tok, const uint32_t *__restrict__ rec_cnt,
                                        const uint32_t *__restrict__ row_off, const uint32_t *__restrict__ row_rec,
                                        int64_t g, int64_t G, const RowOut &out, const uint32_t *late_bits,
                                        int lane) {
    const int S = P.S;
    const bool vec = (S & 3) == 0;  // 16-byte aligned rows
    const bool vec_lb = (P.label_width & 3) == 0;
    const DirectDst &dd = out.direct;
    int32_t *ids_o = out.input_ids + g * S;
    int32_t *am_o = out.attention_mask + g * S;
    int32_t *tt_o = out.token_type_ids ? out.token_type_ids + g * S : nullptr;
    int32_t *lb_o = out.labels ? out.labels + g * (int64_t)P.label_width : nullptr;
    if (g < (int64_t)dd.cap) {  // a small push's row: straight into its host batch
        const uint32_t slot = dd.base + (uint32_t)g, bi = slot >= dd.B ? 1u : 0u, row = slot - bi * dd.B;
        ids_o = dd.ids[bi] + (size_t)row * S;
        am_o = dd.am[bi] + (size_t)row * S;
        tt_o = dd.tt[bi] ? dd.tt[bi] + (size_t)row * S : nullptr;
        lb_o = dd.lab[bi] ? dd.lab[bi] + (size_t)row * P.label_width : nullptr;
    }
    if (g >= (int64_t)G) {  // rows of the last batch nobody filled: initial values
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const int j0 = 256 * m + 4 * lane;
            store4(ids_o, j0, S, vec, 0, 0, 0, 0);
            store4(am_o, j0, S, vec, 1, 1, 1, 1);
            if (tt_o) store4(tt_o, j0, S, vec, 0, 0, 0, 0);
            if (lb_o) store4(lb_o, j0, P.label_width, vec_lb, -100, -100, -100, -100);
        }
        return;
    }
    // (LISTS) the row's first chunk c and the boundaries from it on, lane b's chunk_off[c + b]:
    // loaded here, beside the record's fields, not after them (every row has a valid c)
    const int64_t nl = LISTS ? src.n_lists : 0;
    uint32_t c = 0, bnd = 0;  // bnd(0) <= the row's first id < bnd(1)
    if constexpr (LISTS) {
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)src.row_chunk[g]);
        bnd = src.chunk_off[(int64_t)c + lane < nl ? (int64_t)c + lane : nl];
    }
    const int64_t r = row_rec[g];
    const uint32_t k = (uint32_t)(g - row_off[r]);
    const uint32_t cnt = rec_cnt[r];
    const uint32_t t0 = rec_tok[r];
    const int64_t n = (int64_t)cnt + P.n_pre + P.n_post;
    const int64_t base = P.chunk ? (int64_t)k * S : 0;
    const int l = (int)((n - base) < S ? (n - base) : S);
    // (rng_mode 1) the row's mask words, one dword a lane: walked beside the tokenizer
    // (k_mask_bits_rec), else by the LATE pass (late_bits, LDS).  A row the first pass leaves to
    // the LATE one returns only after its loads are issued: the mask words' load, a dependent
    // step after row_rec / row_off, then overlaps the ids' (wave-uniform: a wave per row).
    uint32_t mwd[MR];
    bool mine = true;
    if (RM1) {
        const int64_t pre = rand_pre_slot(P, r, k);
        mine = LATE || pre >= 0;
        const uint32_t *bw = LATE ? late_bits : P.mask_bits0 + (pre >= 0 ? pre : 0) * (int64_t)P.mask_w;
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const int j0 = 256 * m + 4 * lane;
            mwd[m] = j0 < S && mine ? bw[j0 >> 5] : 0u;
        }
        if (LATE) __builtin_amdgcn_wave_barrier();  // (the LDS bits are rewritten by the wave's next rows)
    }

    const RowIds<MR> ids = row_ids<MR, LISTS>(P, src, c, bnd, nl, t0, cnt, base, l, lane);
    const int32_t (&id)[MR][4] = ids.v;
    if (RM1 && !mine) return;  // (the LATE pass's row)
    // attention: 0 on [S-l, S) when l < S (reversed-range quirk, bert_data.rs:58-63 / gpt_data.rs:33-41)
    const int tail0 = l < S ? S - l : S;
    const uint64_t rec = P.first_record + (uint64_t)r;
    if (P.task == 0) {  // MLM: BertData::mask_batch
        bool sel[MR][4];
        if (RM1) {  // rand-compatible mode: the row's bits from k_mask_rand
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                const int j0 = 256 * m + 4 * lane;
#pragma unroll
                for (int w = 0; w < 4; ++w) sel[m][w] = (mwd[m] >> ((j0 + w) & 31)) & 1u;
            }
        } else {
            uint32_t key[MR][4];
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                const uint4 c = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), k, (uint32_t)rec,
                                                         (uint32_t)(rec >> 32)),
                                              (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
                const int j0 = 256 * m + 4 * lane;
                key[m][0] = j0 < S ? c.x : 0xFFFFFFFFu;
                key[m][1] = j0 + 1 < S ? c.y : 0xFFFFFFFFu;
                key[m][2] = j0 + 2 < S ? c.z : 0xFFFFFFFFu;
                key[m][3] = j0 + 3 < S ? c.w : 0xFFFFFFFFu;
            }
            select_k_smallest_interp<MR>(key, P.mask_length, S < 256 * MR ? S : 256 * MR, sel);
        }
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const int j0 = 256 * m + 4 * lane;
            int32_t v[4], lab[4], am[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                v[w] = id[m][w];
                lab[w] = -100;
                if (sel[m][w] && v[w] != 0) {
                    lab[w] = v[w];
                    v[w] = P.mask_id;
                }
                am[w] = j0 + w >= tail0 ? 0 : 1;
            }
            store4(ids_o, j0, S, vec, v[0], v[1], v[2], v[3]);
            store4(am_o, j0, S, vec, am[0], am[1], am[2], am[3]);
            if (tt_o) store4(tt_o, j0, S, vec, 0, 0, 0, 0);
            store4(lb_o, j0, P.label_width, vec_lb, lab[0], lab[1], lab[2], lab[3]);
        }
    } else if (P.task == 3 || P.task == 4) {  // Multi/SingleClass: BertData::put_data rows; labels by k_*_labels
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const int j0 = 256 * m + 4 * lane;
            int32_t am[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) am[w] = j0 + w >= tail0 ? 0 : 1;
            store4(ids_o, j0, S, vec, id[m][0], id[m][1], id[m][2], id[m][3]);
            store4(am_o, j0, S, vec, am[0], am[1], am[2], am[3]);
            if (tt_o) store4(tt_o, j0, S, vec, 0, 0, 0, 0);
        }
    } else {  // CLM: GptData::put_data, labels = row as i32 (no shift)
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const int j0 = 256 * m + 4 * lane;
            int32_t am[4], lab[4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const bool tail = j0 + w >= tail0;
                am[w] = tail ? 0 : 1;
                lab[w] = tail ? -100 : id[m][w];
            }
            store4(ids_o, j0, S, vec, id[m][0], id[m][1], id[m][2], id[m][3]);
            store4(am_o, j0, S, vec, am[0], am[1], am[2], am[3]);
            if (tt_o) store4(tt_o, j0, S, vec, 0, 0, 0, 0);
            store4(lb_o, j0, P.label_width, vec_lb, lab[0], lab[1], lab[2], lab[3]);
        }
    }
}

// ---------------------------------------------------------------------------
// The lean rows (k_rows_fast; DESIGN.md §3 "Lean rows").  k_rows is bound by scalar issue, not by
// its bytes: row_one tests S, the label width, the host destination and the task again at every
// plane store, and its row-invariant fields do not fit the SGPRs.  row_fast_one is the same row for
// the calls launch_rows can promise more about -- S a multiple of 4 (every plane store one 16-byte
// write), no host destination, the Philox contract, the task known at compile time:
//   - a round of 256 positions is bounded once a row, and only the rounds that can pass S at all;
//   - the token-type pointer is tested once a row;
//   - the kernel's arguments are read where a row uses them (RowArgs), not kept across the row;
//   - every id is loaded from a slot clamped into the row's own ids and selected afterwards, and
//     the frame ids are selects: no exec-masked block a load.
// Results are row_one's, bit for bit.
// ---------------------------------------------------------------------------
constexpr int ROW_MLM = 0, ROW_CLM = 1, ROW_LABELS = 2;  // multi-label / single-class: no label plane here

// The kernel's argument where the hardware put it (the kernarg segment, constant address space).
// Taken by value its row-invariant fields are all loaded before the row loop, and those that do
// not fit the SGPRs are moved to VGPR lanes and back a dword an instruction; read through this
// pointer, made opaque again (row_args_again) before each part of a row, a part's fields come
// back by a few scalar loads of up to eight dwords each, from the scalar cache.
typedef const __attribute__((address_space(4))) RowsFastArgs *RowArgs;
__device__ __forceinline__ RowArgs row_args_again(RowArgs a) {
    asm volatile("" : "+s"(a));
    return a;
}

__device__ __forceinline__ void store4v(int32_t *p, int j0, int32_t a, int32_t b, int32_t c, int32_t d) {
    typedef int32_t v4i __attribute__((ext_vector_type(4)));
    __builtin_nontemporal_store(v4i{a, b, c, d}, reinterpret_cast<v4i *>(p + j0));
}

// row_ids for the lean rows.  Position j of the row holds an id when jlo <= j < jhi; lane positions
// outside are clamped into that range before anything is addressed, so every load reads one of the
// row's own ids (a row without ids loads nothing) and the clamped value is dropped by a select.
template <int MR, bool LISTS>
__device__ __forceinline__ RowIds<MR> row_ids_fast(RowArgs a, uint32_t c, uint32_t bnd, int64_t nl, uint32_t t0,
                                                   uint32_t cnt, int64_t base, int l, int lane) {
    const int n_pre = a->F.n_pre;
    const int64_t rel0 = base > n_pre ? base - n_pre : 0;
    const int64_t rel1 = base + l - n_pre < (int64_t)cnt ? base + l - n_pre : (int64_t)cnt;
    const int jlo = (int)(rel0 + n_pre - base), jhi = (int)(rel1 + n_pre - base);
    const uint32_t tb = t0 + (uint32_t)(base - n_pre);  // id index of position 0 (mod 2^32; exact on [jlo, jhi))
    RowIds<MR> out;
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) out.v[m][w] = 0;
    if (rel0 < rel1) {  // (wave-uniform) the row has ids: 0 <= jlo < jhi <= l
        uint32_t t[MR][4];
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int j = 256 * m + 4 * lane + w;
                const int jc = j < jlo ? jlo : j > jhi - 1 ? jhi - 1 : j;
                t[m][w] = tb + (uint32_t)jc;
            }
        if constexpr (LISTS) {
            const uint32_t t_last = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tb + (uint32_t)(jhi - 1)));
            const uint16_t *__restrict__ lc = a->tok.lists + (int64_t)c * STAGE;
            if ((uint32_t)__builtin_amdgcn_readlane((int)bnd, 63) > t_last) {
                uint32_t q[MR][4];  // boundaries at or below the id: its chunk is c + q
#pragma unroll
                for (int m = 0; m < MR; ++m)
#pragma unroll
                    for (int w = 0; w < 4; ++w) q[m][w] = 0;
#pragma unroll 1
                for (int b = 1; b < 64; ++b) {
                    const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)bnd, b);
                    if (x > t_last) break;
#pragma unroll
                    for (int m = 0; m < MR; ++m)
#pragma unroll
                        for (int w = 0; w < 4; ++w) q[m][w] += t[m][w] >= x ? 1u : 0u;
                }
#pragma unroll
                for (int m = 0; m < MR; ++m)
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        // (q <= the boundaries walked: chunk c + q holds id t, at t - its offset)
                        const uint32_t lo = (uint32_t)__shfl((int)bnd, (int)(q[m][w] & 63u));
                        out.v[m][w] = (int32_t)lc[q[m][w] * (uint32_t)STAGE + (t[m][w] - lo)];
                    }
            } else {
                // (a row past the 63 loaded boundaries: one position of every lane a step)
                const uint32_t *const chunk_off = a->tok.chunk_off;
                const uint16_t *const lists = a->tok.lists;
#pragma unroll 1
                for (int i = 0; i < 4 * MR; ++i) {
                    uint32_t ti = 0;
#pragma unroll
                    for (int m = 0; m < MR; ++m)
#pragma unroll
                        for (int w = 0; w < 4; ++w) ti = i == 4 * m + w ? t[m][w] : ti;
                    const int64_t cc = list_chunk_of(chunk_off, (int64_t)c, nl - 1, ti);
                    const int32_t v = (int32_t)lists[list_slot(chunk_off, cc, ti)];
#pragma unroll
                    for (int m = 0; m < MR; ++m)
#pragma unroll
                        for (int w = 0; w < 4; ++w) out.v[m][w] = i == 4 * m + w ? v : out.v[m][w];
                }
            }
        } else {
            const uint32_t *const tok = a->tok.tok;
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int w = 0; w < 4; ++w) out.v[m][w] = (int32_t)tok[t[m][w]];
        }
    }
    // before the ids the opening frame (lane 0's first positions: jlo <= n_pre <= MAX_FRAME), after
    // them the closing one, past the row's l positions 0
    a = row_args_again(a);
    static_assert(MAX_FRAME == 4, "the frame selects below");
    int32_t p0 = a->F.pre[0], p1 = a->F.pre[1], p2 = a->F.pre[2], p3 = a->F.pre[3];
    int32_t q0 = a->F.post[0], q1 = a->F.post[1], q2 = a->F.post[2], q3 = a->F.post[3];
    // (plain SGPR values to the optimizer: a select between loaded values is turned into a branch)
    asm volatile("" : "+s"(p0), "+s"(p1), "+s"(p2), "+s"(p3), "+s"(q0), "+s"(q1), "+s"(q2), "+s"(q3));
    // (every arm a value at hand, one select a statement: nested, the chain stays a branch)
    auto frame4 = [](int k, int32_t x0, int32_t x1, int32_t x2, int32_t x3) {
        int32_t x = x3;
        x = k == 2 ? x2 : x;
        x = k == 1 ? x1 : x;
        x = k == 0 ? x0 : x;
        return x;
    };
    const int post0 = (int)(base - n_pre - (int64_t)cnt);  // (+ j: the closing frame's index)
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int j = 256 * m + 4 * lane + w;
            int32_t v = out.v[m][w];
            if (m == 0) {
                const int32_t f = frame4((int)base + j, p0, p1, p2, p3);
                v = j < jlo ? f : v;
            }
            const int32_t f = frame4(post0 + j, q0, q1, q2, q3);
            v = j >= jhi ? f : v;
            out.v[m][w] = j < l ? v : 0;
        }
    return out;
}

// Round m of a lean row (positions 256 m + 4 lane + w) lies below S: rounds under MR / 2 always do
// (MR is the power of two at or above ceil(S / 256)); S % 4 == 0, so a lane's four positions pass S
// together.
template <int MR>
struct RowIn {
    bool r[MR];
};
template <int MR>
__device__ __forceinline__ RowIn<MR> row_in(int S, int lane) {
    RowIn<MR> x;
#pragma unroll
    for (int m = 0; m < MR; ++m) x.r[m] = m < MR / 2 || 256 * m + 4 * lane < S;
    return x;
}

// the planes of one lean row, every round's stores under its one bound; the token-type plane's
// zeros behind one test of its pointer
template <int MR, int TASK>
__device__ __forceinline__ void row_fast_store(RowArgs a, uint32_t g, int lane, const int32_t (&v)[MR][4],
                                               const int32_t (&am)[MR][4], const int32_t (&lab)[MR][4]) {
    a = row_args_again(a);
    const int S = a->F.S;
    const RowIn<MR> in = row_in<MR>(S, lane);
    const int64_t o = (int64_t)g * S;
    int32_t *const ids_o = a->F.input_ids + o, *const am_o = a->F.attention_mask + o;
    int32_t *const lb_o = TASK != ROW_LABELS ? a->F.labels + o : nullptr;
    int32_t *const tt = a->F.token_type_ids;
#pragma unroll
    for (int m = 0; m < MR; ++m)
        if (in.r[m]) {
            const int j0 = 256 * m + 4 * lane;
            store4v(ids_o, j0, v[m][0], v[m][1], v[m][2], v[m][3]);
            store4v(am_o, j0, am[m][0], am[m][1], am[m][2], am[m][3]);
            if constexpr (TASK != ROW_LABELS) store4v(lb_o, j0, lab[m][0], lab[m][1], lab[m][2], lab[m][3]);
        }
    if (tt) {
#pragma unroll
        for (int m = 0; m < MR; ++m)
            if (in.r[m]) store4v(tt + o, 256 * m + 4 * lane, 0, 0, 0, 0);
    }
}

// row_one for the lean kernels: row g of the call (a wave), g >= G a padding row of the last batch.
template <int MR, int TASK, bool LISTS>
__device__ __forceinline__ void row_fast_one(RowArgs a, uint32_t g, uint32_t G, int lane) {
    int32_t v[MR][4], am[MR][4], lab[MR][4];
    if (g >= G) {  // rows of the last batch nobody filled: initial values
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                v[m][w] = 0;
                am[m][w] = 1;
                lab[m][w] = -100;
            }
        row_fast_store<MR, TASK>(a, g, lane, v, am, lab);
        return;
    }
    a = row_args_again(a);
    const int S = a->F.S;
    const int64_t nl = LISTS ? a->tok.n_lists : 0;
    uint32_t c = 0, bnd = 0;  // (LISTS, as row_one) bnd(0) <= the row's first id < bnd(1)
    if constexpr (LISTS) {
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)a->tok.row_chunk[g]);
        bnd = a->tok.chunk_off[(int64_t)c + lane < nl ? (int64_t)c + lane : nl];
    }
    const uint32_t r = a->row_rec[g];
    const uint32_t k = g - a->row_off[r];
    const uint32_t cnt = a->rec_cnt[r];
    const uint32_t t0 = a->rec_tok[r];
    const int64_t n = (int64_t)cnt + a->F.n_pre + a->F.n_post;
    const int64_t base = a->F.chunk ? (int64_t)k * S : 0;
    const int l = (int)((n - base) < S ? (n - base) : S);
    const RowIds<MR> ids = row_ids_fast<MR, LISTS>(a, c, bnd, nl, t0, cnt, base, l, lane);
    const int32_t (&id)[MR][4] = ids.v;
    // attention: 0 on [S-l, S) when l < S (reversed-range quirk, as row_one)
    const int tail0 = l < S ? S - l : S;
    if constexpr (TASK == ROW_MLM) {  // BertData::mask_batch
        a = row_args_again(a);
        const uint64_t rec = a->F.first_record + (uint64_t)r;
        const uint64_t seed = a->F.seed;
        const RowIn<MR> in = row_in<MR>(S, lane);
        uint32_t key[MR][4];
        bool sel[MR][4];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const uint4 x = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), k, (uint32_t)rec, (uint32_t)(rec >> 32)),
                                          (uint32_t)seed, (uint32_t)(seed >> 32));
            key[m][0] = in.r[m] ? x.x : 0xFFFFFFFFu;
            key[m][1] = in.r[m] ? x.y : 0xFFFFFFFFu;
            key[m][2] = in.r[m] ? x.z : 0xFFFFFFFFu;
            key[m][3] = in.r[m] ? x.w : 0xFFFFFFFFu;
        }
        select_k_smallest_interp<MR>(key, a->F.mask_length, S, sel);
        a = row_args_again(a);
        const int32_t mask_id = a->F.mask_id;
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const bool pick = sel[m][w] && id[m][w] != 0;
                v[m][w] = pick ? mask_id : id[m][w];
                lab[m][w] = pick ? id[m][w] : -100;
                am[m][w] = 256 * m + 4 * lane + w >= tail0 ? 0 : 1;
            }
    } else {  // CLM: GptData::put_data, labels = row as i32 (no shift); the label tasks: BertData::put_data rows
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const bool tail = 256 * m + 4 * lane + w >= tail0;
                v[m][w] = id[m][w];
                am[m][w] = tail ? 0 : 1;
                lab[m][w] = tail ? -100 : id[m][w];
            }
    }
    row_fast_store<MR, TASK>(a, g, lane, v, am, lab);
}

// ---------------------------------------------------------------------------
// The BERT masking policies (sdl_config.mask_policy 1 / 2; DESIGN.md §3 "Masking policies").
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t max_u32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t min_u32r(uint32_t a, uint32_t b) { return a < b ? a : b; }
// the wave, as mlm_pick.hpp asks for it: sums and minima over all lanes, uniform
struct PickWave {
    uint32_t l;
    __device__ __forceinline__ uint32_t sum(uint32_t x) const {
        return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_sum(x), 63);
    }
    __device__ __forceinline__ uint32_t min(uint32_t x) const {
        DPP_SCAN_ID(x, min_u32r, 0xFFFFFFFFu);
        return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    }
    __device__ __forceinline__ uint32_t lane() const { return l; }
};

// One MLM row g under policy 1 (WHOLE = false: every candidate a unit) or 2 (whole words), a wave:
// row_one's geometry, framing, attention and stores; the pick and the 80/10/10 replacement are
// the contract's.  A lane's masks are a bit per element, bit 4 m + w = position 256 m + 4 lane + w.
// WHOLE: `lds` is the wave's 256 MR words -- the units' sizes (counted into their first position)
// and then their picked flags, read back by the unit's other positions.
template <int MR, bool WHOLE, bool LISTS>
__device__ __forceinline__ void row_policy_one(const RowParams &P, const MaskPolicy &mp, const TokSrc &src,
                                               const uint32_t *__restrict__ rec_tok,
                                               const uint32_t *__restrict__ rec_cnt,
                                               const uint32_t *__restrict__ row_off,
                                               const uint32_t *__restrict__ row_rec, int64_t g, int64_t G,
                                               const RowOut &out, uint32_t *lds, int lane) {
    const int S = P.S;
    const bool vec = (S & 3) == 0;
    const DirectDst &dd = out.direct;
    int32_t *ids_o = out.input_ids + g * S;
    int32_t *am_o = out.attention_mask + g * S;
    int32_t *tt_o = out.token_type_ids ? out.token_type_ids + g * S : nullptr;
    int32_t *lb_o = out.labels + g * (int64_t)S;  // (mlm: label_width = S)
    if (g < (int64_t)dd.cap) {  // a small push's row: straight into its host batch
        const uint32_t slot = dd.base + (uint32_t)g, bi = slot >= dd.B ? 1u : 0u, row = slot - bi * dd.B;
        ids_o = dd.ids[bi] + (size_t)row * S;
        am_o = dd.am[bi] + (size_t)row * S;
        tt_o = dd.tt[bi] ? dd.tt[bi] + (size_t)row * S : nullptr;
        lb_o = dd.lab[bi] + (size_t)row * S;
    }
    if (g >= (int64_t)G) {  // rows of the last batch nobody filled: initial values
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const int j0 = 256 * m + 4 * lane;
            store4(ids_o, j0, S, vec, 0, 0, 0, 0);
            store4(am_o, j0, S, vec, 1, 1, 1, 1);
            if (tt_o) store4(tt_o, j0, S, vec, 0, 0, 0, 0);
            store4(lb_o, j0, S, vec, -100, -100, -100, -100);
        }
        return;
    }
    const int64_t nl = LISTS ? src.n_lists : 0;
    uint32_t c = 0, bnd = 0;
    if constexpr (LISTS) {
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)src.row_chunk[g]);
        bnd = src.chunk_off[(int64_t)c + lane < nl ? (int64_t)c + lane : nl];
    }
    const int64_t r = row_rec[g];
    const uint32_t ck = (uint32_t)(g - row_off[r]);  // the row's chunk of its record
    const uint32_t cnt = rec_cnt[r];
    const uint32_t t0 = rec_tok[r];
    const int64_t n = (int64_t)cnt + P.n_pre + P.n_post;
    const int64_t base = P.chunk ? (int64_t)ck * S : 0;
    const int l = (int)((n - base) < S ? (n - base) : S);
    const RowIds<MR> ids = row_ids<MR, LISTS>(P, src, c, bnd, nl, t0, cnt, base, l, lane);
    const int32_t (&id)[MR][4] = ids.v;
    const int tail0 = l < S ? S - l : S;
    const uint64_t rec = P.first_record + (uint64_t)r;
    const PickWave wv{(uint32_t)lane};

    // candidates: filled positions whose id is none of 0, mask_id and the framing ids
    uint32_t cand = 0;
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int32_t v = id[m][w];
            bool ex = v == 0 || v == P.mask_id;
#pragma unroll
            for (int q = 0; q < MAX_FRAME; ++q)
                ex = ex || (q < P.n_pre && v == frame_id(P.pre, q)) || (q < P.n_post && v == frame_id(P.post, q));
            if (256 * m + 4 * lane + w < l && !ex) cand |= 1u << (4 * m + w);
        }
    const int ncand = (int)wv.sum((uint32_t)__popc(cand));
    int kb = (int)(((int64_t)l * mp.per_mille + 500) / 1000);
    kb = kb < 1 ? 1 : kb;
    kb = kb < P.mask_length ? kb : P.mask_length;
    if (ncand == 0) kb = 0;

    uint32_t sel = 0;  // the picked positions
    if (kb > 0) {  // (wave-uniform)
        uint32_t key[4 * MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const uint4 x = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), ck, (uint32_t)rec, (uint32_t)(rec >> 32)),
                                          (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
            key[4 * m] = x.x;
            key[4 * m + 1] = x.y;
            key[4 * m + 2] = x.z;
            key[4 * m + 3] = x.w;
        }
        if constexpr (!WHOLE) {
            // the kb smallest keys among the candidates (all of them if fewer): k_rows' select on
            // keys pushed to the top off the candidates.  (A candidate whose own key is
            // 0xFFFFFFFF would tie with those; 2^-32 a position, and no input steers a Philox word.)
            uint32_t k2[MR][4];
            bool s2[MR][4];
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int w = 0; w < 4; ++w) k2[m][w] = (cand >> (4 * m + w)) & 1u ? key[4 * m + w] : 0xFFFFFFFFu;
            select_k_smallest_interp<MR>(k2, kb < ncand ? kb : ncand, ncand, s2);
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int w = 0; w < 4; ++w) sel |= s2[m][w] ? 1u << (4 * m + w) : 0u;
            sel &= cand;
        } else {
            auto step = [] {  // one lane's LDS writes before the others' reads (a wave: program order)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            };
            // continuation bits of the candidates' ids (the bitmap: 4 KiB for 30522 ids, L2-resident)
            uint32_t cont = 0;
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e) {
                const uint32_t v = (uint32_t)id[e >> 2][e & 3];
                const uint32_t wd = (cand >> e) & 1u && v < mp.vocab_size ? mp.cont_bits[v >> 5] : 0u;
                cont |= ((wd >> (v & 31u)) & 1u) << e;
            }
            // is position j - 1 a candidate: the lane's own lower element, the previous lane's
            // last of the round, or (lane 0) lane 63's last of the round before
            const uint32_t xp = wave_prev(cand), x63 = (uint32_t)__builtin_amdgcn_readlane((int)cand, 63);
            const uint32_t prev = ((cand << 1) & 0xEEEEEEEEu) |
                                  (lane > 0 ? (xp >> 3) & 0x11111111u : (x63 << 1) & 0x11111110u);
            const uint32_t start = cand & ~(cont & prev);
            // every position's unit: the last start at or before it (position + 1; a max-scan,
            // lane-local, then over the wave, carried across the rounds), counted into its size
#pragma unroll
            for (int m = 0; m < MR; ++m)
#pragma unroll
                for (int w = 0; w < 4; ++w) lds[256 * m + 4 * lane + w] = 0u;
            step();
            uint32_t us[4 * MR], carry = 0;
#pragma unroll
            for (int m = 0; m < MR; ++m) {
                uint32_t a[4], run = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    run = (start >> (4 * m + w)) & 1u ? (uint32_t)(256 * m + 4 * lane + w) + 1u : run;
                    a[w] = run;
                }
                uint32_t incl = run;
                DPP_SCAN(incl, max_u32);
                const uint32_t before = max_u32(carry, wave_prev(incl));
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    us[4 * m + w] = max_u32(before, a[w]);  // (a candidate always has one: never 0 there)
                    if ((cand >> (4 * m + w)) & 1u) atomicAdd(&lds[us[4 * m + w] ? us[4 * m + w] - 1u : 0u], 1u);
                }
                carry = max_u32(carry, (uint32_t)__builtin_amdgcn_readlane((int)incl, 63));
            }
            step();
            uint32_t size[4 * MR];
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e)
                size[e] = (start >> e) & 1u ? lds[256 * (e >> 2) + 4 * lane + (e & 3)] : 0u;
            const uint32_t taken = mlm_pick_units<4 * MR>(key, size, (uint32_t)kb, wv);
            step();
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e)
                if ((start >> e) & 1u) lds[256 * (e >> 2) + 4 * lane + (e & 3)] = (taken >> e) & 1u;
            step();
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e)
                if ((cand >> e) & 1u) sel |= (lds[us[e] ? us[e] - 1u : 0u] & 1u) << e;
            step();  // (the wave's next row rewrites the LDS)
        }
    }
    // labels and the replacement: 80 % mask_id, 10 % a random id, 10 % unchanged, drawn only by
    // the lanes that own a picked position
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        const int j0 = 256 * m + 4 * lane;
        const uint32_t s4 = (sel >> (4 * m)) & 15u;
        int32_t v[4], lab[4], am[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            v[w] = id[m][w];
            lab[w] = -100;
            am[w] = j0 + w >= tail0 ? 0 : 1;
        }
        if (s4) {
            const uint4 u4 = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), ck | 0x20000000u, (uint32_t)rec,
                                                      (uint32_t)(rec >> 32)),
                                           (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
            const uint32_t u[4] = {u4.x, u4.y, u4.z, u4.w};
            bool any_rand = false;
#pragma unroll
            for (int w = 0; w < 4; ++w)
                any_rand = any_rand || ((s4 >> w) & 1u && u[w] >= 0xCCCCCCCDu && u[w] < 0xE6666667u);
            uint32_t rr[4] = {0u, 0u, 0u, 0u};
            if (any_rand) {
                const uint4 r4 = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), ck | 0x30000000u, (uint32_t)rec,
                                                          (uint32_t)(rec >> 32)),
                                               (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
                rr[0] = r4.x;
                rr[1] = r4.y;
                rr[2] = r4.z;
                rr[3] = r4.w;
            }
#pragma unroll
            for (int w = 0; w < 4; ++w)
                if ((s4 >> w) & 1u) {
                    lab[w] = v[w];
                    if (u[w] < 0xCCCCCCCDu) v[w] = P.mask_id;
                    else if (u[w] < 0xE6666667u) v[w] = (int32_t)__umulhi(rr[w], mp.vocab_size);
                }
        }
        store4(ids_o, j0, S, vec, v[0], v[1], v[2], v[3]);
        store4(am_o, j0, S, vec, am[0], am[1], am[2], am[3]);
        if (tt_o) store4(tt_o, j0, S, vec, 0, 0, 0, 0);
        store4(lb_o, j0, S, vec, lab[0], lab[1], lab[2], lab[3]);
    }
}

// A per-record push (<= 64 records, <= 64 chunks): the same steps on one wave -- wave scans, no
// workgroup barriers.  With the rows fused (MR > 0: nothing after this kernel reads the call's
// record / row tables) those tables live in LDS, so the only global round trip between steps is
// the compacted ids (a push is bound by such dependent round trips: 10.6 us with every table in
// global memory).  Lane order is program order within the wave; a fence between steps makes one
// lane's writes visible to the others' reads.
template <int MR>
__device__ __forceinline__ void downstream_tiny(const SmallDown &d, const RowParams &P, const uint64_t *__restrict__ off,
                                                int64_t R, int64_t N, int64_t n_chunks) {
    constexpr int ROWS_LDS = 1024;
    __shared__ uint32_t s_coff[65], s_rtok[64], s_rcnt[64], s_rrows[64], s_roff[65];
    __shared__ uint32_t s_rrec[MR > 0 ? ROWS_LDS : 1];
    const int lane = lane_id();
    auto step = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    uint32_t *const coff = MR > 0 ? s_coff : d.chunk_off;
    uint32_t *const rtok = MR > 0 ? s_rtok : d.rec_tok, *const rcnt = MR > 0 ? s_rcnt : d.rec_cnt;
    uint32_t *const rrows = MR > 0 ? s_rrows : d.rec_rows, *const roff = MR > 0 ? s_roff : d.row_off;
    {
        const uint32_t c = lane < n_chunks ? d.chunk_cnt[lane] : 0u;
        const uint32_t incl = wave_incl_sum(c);
        if (lane < n_chunks) coff[lane] = incl - c;
        if (lane == 63) coff[n_chunks] = incl;
    }
    step();
    // (the records' loads before the compaction's stores: independent, in flight together)
    if (lane < R) record_one(P, off, lane, N, coff, n_chunks, d.rec_local, rtok, rcnt, rrows);
    for (int64_t cb = 0; cb < n_chunks; cb += COMPACT_CPW) compact_small(d, cb, coff, n_chunks);
    step();
    uint32_t G;
    {
        const uint32_t c = lane < R ? rrows[lane] : 0u;
        const uint32_t incl = wave_incl_sum(c);
        G = (uint32_t)lane_bcast((int)incl, 63);
        if (lane < R) roff[lane] = incl - c;
        if (lane == 63) roff[R] = incl;
        uint32_t *const rrec = MR > 0 && G <= (uint32_t)ROWS_LDS ? s_rrec : d.row_rec;
        if (lane < R)
            for (uint32_t g = incl - c; g < incl; ++g) rrec[g] = (uint32_t)lane;
        if (d.stat) {
            if (lane < R) d.stat[lane] = incl - c;
            if (lane == 63) {
                d.stat[R] = incl;
                d.stat[R + 1] = 0u;
                d.stat[R + 2] = d.tok_err ? *d.tok_err : 0u;  // a t5 tokenizer under mlm / clm
            }
        }
    }
    if constexpr (MR > 0) {
        step();
        const uint32_t *const rrec = G <= (uint32_t)ROWS_LDS ? s_rrec : d.row_rec;
        const int64_t g_end = d.out.direct.cap ? (int64_t)G : ((int64_t)G + P.B - 1) / P.B * P.B;
        for (int64_t g = 0; g < g_end; ++g)
            row_one<MR, false, false>(P, TokSrc{d.tok}, rtok, rcnt, roff, rrec, g, (int64_t)G, d.out, nullptr, lane);
    }
}

}  // namespace sdl
