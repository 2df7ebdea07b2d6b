// pack_mlm_bpe.hip -- MLM rows packed from the concatenated document stream over a byte-level BPE
// tokenizer in RoBERTa's form (sdl_config.pack = 1 under the MLM task, DESIGN.md §3 "Packed mlm
// rows") on gfx950: RoBERTa's FULL-SENTENCES rows with dynamic masking, whole words read from the
// "Ġ" prefix.
//
// The call's stream is  carry ++ concat over kept records r of ([<s>] ++ ids_r ++ [</s>]),  pk_off[r]
// the stream position where record r starts, and row g of the call is stream[g S, (g + 1) S).
// pack_mlm.hip finds every column's record with a search per lane and walks the WordPiece chunk
// lists; here the ids are a dense array, so the only thing a column needs is its document, and a
// wave builds that once for its row as a segment table in LDS:
//
//   1. one wave-uniform binary search in pk_off: the record of the row's first position past the carry;
//   2. from there the lanes load 64 consecutive pk_off entries at a time, coalesced; a record of
//      length > 0 that starts inside the row is kept (dropped records share an offset and give no
//      segment), a ballot and mbcnt rank the kept ones in order, and record k of the row writes
//      seg[k] = (start column, rec_tok - start column) and sets its start bit in the row's bitmap
//      (S <= 2048 bits: one 32-bit word a lane).  The record already open at column 0 is entry 0;
//      the first boundary at or past the row's end closes the table as its last entry's start;
//   3. a column's segment is the number of start bits at or below it: the wave's inclusive sum of
//      the words' popcounts (DPP), read across lanes through LDS, plus the popcount inside the word.
//
// Column j of segment (c, base) is <s> at j = c, </s> where j - c passes the record's count (the
// next entry's start tells it) and tok[base + j - 1] between; position_id j - max(c, 0).  The four
// ids a lane and round are independent loads.  With the row in registers the wave runs the policy
// contract on it as chunk 0 of record q, the row's packed index on the handle, l = S filled
// positions: candidates are every id but <s>, </s>, <mask> and <pad> -- id 0 is a piece here -- and
// policy 2 joins position j to the unit before it when the word-start bit of its id is clear.  The
// map (<= 8 KiB) is read through global memory: a wave reads it once a row for the candidates'
// ids, it stays in L2, and a copy to LDS would cost every block 8 KiB of the 64 it may declare.
//
// Geometry: k_rows_policy's -- four rows a block, lane L owns columns 256 m + 4 L + w of its row,
// MR rounds of them.  The candidate, key, unit-build, pick and 80/10/10 blocks are copies of
// pack_mlm.hip's (mlm_policy_device.hpp says why they are copies); Philox, the selects, PickWave,
// the budget and the thresholds are that header's.
#include "device_util.hpp"
#include "kernels.hpp"
#include "pack_search.hpp"
#include "rows_device.hpp"

namespace sdl {

// A row holds at most (S - 2) / 3 + 2 segments -- a kept document has >= 3 stream ids, the first
// and the last may be cut -- and one closing entry.
constexpr int pack_bpe_segs(int MR) { return (256 * MR - 2) / 3 + 3; }

// A wave's LDS: the segment table, the bitmap with its exclusive scan, the whole-word build's words.
template <int MR, bool WHOLE>
struct PackBpeLds {
    uint2 seg[pack_bpe_segs(MR)];
    uint32_t bm[64], pre[64];
    uint32_t unit[WHOLE ? 256 * MR : 1];
};
static_assert(4 * sizeof(PackBpeLds<8, true>) <= 65536, "four waves' tables fit the LDS a block may declare");

// one lane's LDS writes before the others' reads (a wave: program order)
__device__ __forceinline__ void wave_lds_step() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// A row nobody filled: the unpacked mlm initial values, position_ids 0.
template <int MR>
__device__ __forceinline__ void pack_bpe_pad_row(const PackMlmBpeParams &q, uint32_t g, int lane) {
    const int S = q.S;
    const bool vec = (S & 3) == 0;
    const size_t o = (size_t)g * S;
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        const int j0 = 256 * m + 4 * lane;
        store4(q.ids + o, j0, S, vec, 0, 0, 0, 0);
        store4(q.am + o, j0, S, vec, 1, 1, 1, 1);
        store4(q.tt + o, j0, S, vec, 0, 0, 0, 0);
        store4(q.lab + o, j0, S, vec, -100, -100, -100, -100);
        store4(q.pos + o, j0, S, vec, 0, 0, 0, 0);
    }
}

// Output row g = stream[row0, row0 + l) (l = S; the flush row: row0 = 0 and l = c0, all of it the
// carry), masked as chunk 0 of record `rec`; columns >= l: <pad>, attention 0, labels -100.
template <int MR, bool WHOLE>
__device__ __forceinline__ void pack_bpe_row(const PackMlmBpeParams &q, uint32_t g, uint32_t row0, int l, uint32_t c0,
                                             uint64_t rec, PackBpeLds<MR, WHOLE> &sm, int lane) {
    constexpr uint32_t NSEG = (uint32_t)pack_bpe_segs(MR);
    const int S = q.S;
    const bool vec = (S & 3) == 0;
    int32_t *ids_o = q.ids + (size_t)g * S;
    int32_t *am_o = q.am + (size_t)g * S;
    int32_t *tt_o = q.tt + (size_t)g * S;
    int32_t *lb_o = q.lab + (size_t)g * S;
    int32_t *ps_o = q.pos + (size_t)g * S;

    // ---- the segment table of the row's part past the carry (wave-uniform control flow) ----
    const uint32_t rowend = row0 + (uint32_t)l;
    const uint32_t wf = row0 > c0 ? row0 : c0;
    const bool segs = wf < rowend;  // (then R > 0 and rowend <= L = pk_off[R])
    uint32_t open = 0;              // 1: entry 0 is the record open at column 0, which has no start bit
    if (segs) {
        const uint32_t R = (uint32_t)q.R;
        sm.bm[lane] = 0u;
        wave_lds_step();
        uint32_t rb = (uint32_t)__builtin_amdgcn_readfirstlane((int)pack_record_of(q.pk_off, 0u, R - 1u, wf));
        uint32_t K = 0;
        const uint32_t s0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.pk_off[rb]);
        if (s0 < row0) {
            if (lane == 0) sm.seg[0] = make_uint2(s0 - row0, q.rec_tok[rb] - (s0 - row0));
            open = K = 1u;
            ++rb;
        }
        for (;;) {
            const uint32_t r = rb + (uint32_t)lane;  // (r = R: the stream's end, a boundary and no record)
            const uint32_t a = r <= R ? q.pk_off[r] : 0xFFFFFFFFu;
            const uint32_t b = r < R ? q.pk_off[r + 1u] : a;
            const bool keep = r < R && b > a && a < rowend;
            const uint64_t kb = __ballot(keep);
            if (keep) {
                const uint32_t k = K + __builtin_amdgcn_mbcnt_hi((uint32_t)(kb >> 32),
                                                                 __builtin_amdgcn_mbcnt_lo((uint32_t)kb, 0u));
                const uint32_t sc = a - row0;  // (a >= wf >= row0)
                if (k < NSEG - 1u) sm.seg[k] = make_uint2(sc, q.rec_tok[r] - sc);
                atomicOr(&sm.bm[sc >> 5], 1u << (sc & 31u));
            }
            K += (uint32_t)__popcll(kb);
            const uint64_t pb = __ballot(r <= R && a >= rowend);
            const bool last = rb + 63u >= R;  // (the batch held r = R: pb is set, pk_off[R] >= rowend)
            if (pb || last) {
                const uint32_t e = pb ? (uint32_t)__builtin_amdgcn_readlane((int)a, __ffsll((unsigned long long)pb) - 1)
                                      : rowend;
                if (lane == 0 && K < NSEG) sm.seg[K] = make_uint2(e - row0, 0u);
                break;
            }
            rb += 64u;
        }
        wave_lds_step();
        const uint32_t mine = (uint32_t)__popc(sm.bm[lane]);
        sm.pre[lane] = wave_incl_sum(mine) - mine;
        wave_lds_step();
    }

    // ---- columns to ids ----
    int32_t id[MR][4];
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        const int j0 = 256 * m + 4 * lane;
        const int wi = 8 * m + (lane >> 3);  // the bitmap word of the lane's four columns
        uint32_t wd = 0, wp = 0;
        if (segs) {
            wd = sm.bm[wi];
            wp = sm.pre[wi];
        }
        int32_t ps[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int j = j0 + w;
            int32_t v = q.pad, pp = 0;
            if (j < l) {
                const uint32_t p = row0 + (uint32_t)j;
                if (p < c0) {  // (the carry lies in row 0)
                    v = q.carry_ids[p];
                    pp = q.carry_pos[p];
                } else {
                    const uint32_t cnt = wp + (uint32_t)__popc(wd & (0xFFFFFFFFu >> (31 - (j & 31))));
                    uint32_t k = cnt - 1u + open;
                    k = k < NSEG - 2u ? k : NSEG - 2u;  // (a row's segments: never more)
                    const uint2 s = sm.seg[k];
                    const int sc = (int)s.x;
                    const int i = j - sc, n = (int)sm.seg[k + 1u].x - sc - 2;  // the document is <s> ids </s>
                    if (i == 0) v = q.cls;
                    else if (i > n) v = q.sep;
                    else v = (int32_t)q.tok[s.y + (uint32_t)j - 1u];
                    pp = j - (sc > 0 ? sc : 0);
                }
            }
            id[m][w] = v;
            ps[w] = pp;
        }
        store4(ps_o, j0, S, vec, ps[0], ps[1], ps[2], ps[3]);
        store4(tt_o, j0, S, vec, 0, 0, 0, 0);
    }
    const PickWave wv{(uint32_t)lane};

    // candidates: filled positions whose id is none of <s>, </s>, mask_id and <pad> (id 0 is a piece)
    uint32_t cand = 0;
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int32_t v = id[m][w];
            const bool ex = v == q.mask_id || v == q.cls || v == q.sep || v == q.pad;
            if (256 * m + 4 * lane + w < l && !ex) cand |= 1u << (4 * m + w);
        }
    const int ncand = (int)wv.sum((uint32_t)__popc(cand));
    const int kb = policy_budget(l, ncand, q.per_mille, q.mask_length);

    // the pick: row_policy_one's, for chunk 0 of record `rec`
    uint32_t sel = 0;  // the picked positions
    if (kb > 0) {      // (wave-uniform)
        uint32_t key[4 * MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const uint4 x = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), 0u, (uint32_t)rec, (uint32_t)(rec >> 32)),
                                          (uint32_t)q.seed, (uint32_t)(q.seed >> 32));
            key[4 * m] = x.x;
            key[4 * m + 1] = x.y;
            key[4 * m + 2] = x.z;
            key[4 * m + 3] = x.w;
        }
        if constexpr (!WHOLE) {
            // the kb smallest keys among the candidates (all of them if fewer): keys pushed to the
            // top off the candidates
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
            uint32_t *lds = sm.unit;
            // continuation bits of the candidates' ids: the word-start bit clear
            uint32_t cont = 0;
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e) {
                const uint32_t v = (uint32_t)id[e >> 2][e & 3];
                const uint32_t wd = (cand >> e) & 1u && v < q.vocab_size ? q.word_start[v >> 5] : 0xFFFFFFFFu;
                cont |= (~(wd >> (v & 31u)) & 1u) << e;
            }
            // is position j - 1 a candidate: the lane's own lower element, the previous lane's
            // last of the round, or (lane 0) lane 63's last of the round before.  Column 0 has no
            // position before it: a row that begins inside a word starts a unit there.
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
            wave_lds_step();
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
            wave_lds_step();
            uint32_t size[4 * MR];
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e)
                size[e] = (start >> e) & 1u ? lds[256 * (e >> 2) + 4 * lane + (e & 3)] : 0u;
            const uint32_t taken = mlm_pick_units<4 * MR>(key, size, (uint32_t)kb, wv);
            wave_lds_step();
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e)
                if ((start >> e) & 1u) lds[256 * (e >> 2) + 4 * lane + (e & 3)] = (taken >> e) & 1u;
            wave_lds_step();
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e)
                if ((cand >> e) & 1u) sel |= (lds[us[e] ? us[e] - 1u : 0u] & 1u) << e;
        }
    }
    // labels and the replacement: 80 % mask_id, 10 % a random id, 10 % unchanged, drawn only by
    // the lanes that own a picked position; then the three planes left
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        const int j0 = 256 * m + 4 * lane;
        const uint32_t s4 = (sel >> (4 * m)) & 15u;
        int32_t v[4], lab[4], am[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            v[w] = id[m][w];
            lab[w] = -100;
            am[w] = j0 + w < l ? 1 : 0;
        }
        if (s4) {
            const uint4 u4 = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), 0x20000000u, (uint32_t)rec,
                                                      (uint32_t)(rec >> 32)),
                                           (uint32_t)q.seed, (uint32_t)(q.seed >> 32));
            const uint32_t u[4] = {u4.x, u4.y, u4.z, u4.w};
            bool any_rand = false;
#pragma unroll
            for (int w = 0; w < 4; ++w)
                any_rand = any_rand || ((s4 >> w) & 1u && u[w] >= POLICY_MASK_BELOW && u[w] < POLICY_RANDOM_BELOW);
            uint32_t rr[4] = {0u, 0u, 0u, 0u};
            if (any_rand) {
                const uint4 r4 = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), 0x30000000u, (uint32_t)rec,
                                                          (uint32_t)(rec >> 32)),
                                               (uint32_t)q.seed, (uint32_t)(q.seed >> 32));
                rr[0] = r4.x;
                rr[1] = r4.y;
                rr[2] = r4.z;
                rr[3] = r4.w;
            }
#pragma unroll
            for (int w = 0; w < 4; ++w)
                if ((s4 >> w) & 1u) {
                    lab[w] = v[w];
                    if (u[w] < POLICY_MASK_BELOW) v[w] = q.mask_id;
                    else if (u[w] < POLICY_RANDOM_BELOW) v[w] = (int32_t)__umulhi(rr[w], q.vocab_size);
                }
        }
        store4(ids_o, j0, S, vec, v[0], v[1], v[2], v[3]);
        store4(am_o, j0, S, vec, am[0], am[1], am[2], am[3]);
        store4(lb_o, j0, S, vec, lab[0], lab[1], lab[2], lab[3]);
    }
    wave_lds_step();  // (the wave's next row rewrites the LDS)
}

// The five planes of the call's rows: rows [0, G) the stream, [G, end) the padding rows up to the
// next multiple of B.  The grid is sized from the upper bound rows_cap -- the row count stays on
// the device -- and the packed index of row g is the handle's counter (the half the last call
// wrote; k_pack_mlm_bpe_carry writes the other one) plus g.
template <int MR, bool WHOLE>
__global__ __launch_bounds__(256) void k_pack_mlm_bpe_rows(PackMlmBpeParams q) {
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ PackBpeLds<MR, WHOLE> s_wave[4];
    const uint32_t S = (uint32_t)q.S, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / S;
    uint64_t gpad = ((uint64_t)G + (uint64_t)q.B - 1u) / (uint64_t)q.B * (uint64_t)q.B;
    if (gpad > (uint64_t)q.rows_cap) gpad = (uint64_t)q.rows_cap;
    const uint32_t end = (uint32_t)gpad;  // (rows_cap * S < 2^32: checked by the host)
    const uint64_t q0 = *q.row_cnt;
    for (uint32_t g = blockIdx.x * 4u + (uint32_t)wid; g < end; g += gridDim.x * 4u) {
        if (g < G) pack_bpe_row<MR, WHOLE>(q, g, g * S, (int)S, c0, q0 + g, s_wave[wid], lane);
        else pack_bpe_pad_row<MR>(q, g, lane);
    }
}

// stream[G S :) unmasked, with its position_ids in the row it will open -> the other half of the
// carry, the new length, the row counter advanced by G and the call's row count (one workgroup;
// fewer than S <= 2048 elements, a binary search in pk_off each).
__global__ __launch_bounds__(256) void k_pack_mlm_bpe_carry(PackMlmBpeParams q) {
    const uint32_t S = (uint32_t)q.S, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / S, full = G * S, n = L - full;
    for (uint32_t x = threadIdx.x; x < n; x += 256u) {
        const uint32_t p = full + x;
        if (p < c0) {  // (G == 0: the old carry stays in front)
            q.new_ids[x] = q.carry_ids[p];
            q.new_pos[x] = q.carry_pos[p];
        } else {  // (c0 <= p < L: R > 0 and the record has length > 0)
            const uint32_t r = pack_record_of(q.pk_off, 0u, R - 1u, p);
            const uint32_t start = q.pk_off[r], i = p - start, cnt = q.rec_cnt[r];
            int32_t v;
            if (i == 0u) v = q.cls;
            else if (i > cnt) v = q.sep;
            else v = (int32_t)q.tok[q.rec_tok[r] + i - 1u];
            q.new_ids[x] = v;
            q.new_pos[x] = (int32_t)(p - (start > full ? start : full));
        }
    }
    if (threadIdx.x == 0) {
        *q.new_len = n;
        *q.new_row_cnt = *q.row_cnt + G;
        *q.d_rows = G;
    }
}

// The flush row: the carry's c ids in row 0, masked with l = c and the next packed index, <pad> past
// them; rows 1 .. B - 1 (and row 0 when c == 0) get the padding rows' initial values; the other
// half's length becomes 0 and its counter the old one plus the row.
template <int MR, bool WHOLE>
__global__ __launch_bounds__(256) void k_pack_mlm_bpe_flush(PackMlmBpeParams q) {
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ PackBpeLds<MR, WHOLE> s_wave[4];
    const uint32_t c = *q.carry_len;
    const uint64_t q0 = *q.row_cnt;
    const uint32_t end = (uint32_t)((int64_t)q.B < q.rows_cap ? (int64_t)q.B : q.rows_cap);
    for (uint32_t g = blockIdx.x * 4u + (uint32_t)wid; g < end; g += gridDim.x * 4u) {
        if (g == 0u && c > 0u) pack_bpe_row<MR, WHOLE>(q, 0u, 0u, (int)c, c, q0, s_wave[wid], lane);
        else pack_bpe_pad_row<MR>(q, g, lane);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *q.new_len = 0u;
        *q.new_row_cnt = q0 + (c > 0u ? 1u : 0u);
        *q.d_rows = c > 0u ? 1u : 0u;
    }
}

static bool pack_mlm_bpe_ok(const PackMlmBpeParams &q) {
    return q.S >= 3 && q.S <= 2048 && q.B > 0 && q.R >= 0 && q.R < ((int64_t)1 << 32) - 1 && q.rows_cap >= 0 &&
           q.rows_cap * (int64_t)q.S < ((int64_t)1 << 32) && q.policy >= 1 && q.policy <= 2 &&
           (q.policy != 2 || q.word_start) && q.cls >= 0 && q.sep >= 0 && q.pad >= 0 && q.ids && q.am && q.tt &&
           q.lab && q.pos;
}

#define LAUNCH_PACK_BPE(KERNEL, MM)                                                                  \
    do {                                                                                             \
        if (q.policy == 2) hipLaunchKernelGGL((KERNEL<MM, true>), dim3(grid), dim3(256), 0, st, q);  \
        else hipLaunchKernelGGL((KERNEL<MM, false>), dim3(grid), dim3(256), 0, st, q);               \
    } while (0)
#define LAUNCH_PACK_BPE_MR(KERNEL)                   \
    do {                                             \
        const int MR = (q.S + 255) / 256;            \
        if (MR <= 1) LAUNCH_PACK_BPE(KERNEL, 1);      \
        else if (MR <= 2) LAUNCH_PACK_BPE(KERNEL, 2); \
        else if (MR <= 4) LAUNCH_PACK_BPE(KERNEL, 4); \
        else LAUNCH_PACK_BPE(KERNEL, 8);              \
    } while (0)

hipError_t launch_pack_mlm_bpe_rows(const PackMlmBpeParams &q, hipStream_t st) {
    if (!pack_mlm_bpe_ok(q) || (q.R > 0 && (!q.tok || !q.rec_tok || !q.rec_cnt)) || !q.pk_off) return hipErrorInvalidValue;
    const int64_t want = (q.rows_cap + 3) / 4;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 16384 ? want : 16384);
    LAUNCH_PACK_BPE_MR(k_pack_mlm_bpe_rows);
    hipLaunchKernelGGL(k_pack_mlm_bpe_carry, dim3(1), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t launch_pack_mlm_bpe_flush(const PackMlmBpeParams &q, hipStream_t st) {
    if (!pack_mlm_bpe_ok(q)) return hipErrorInvalidValue;
    const int64_t want = ((int64_t)q.B + 3) / 4;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 4096 ? want : 4096);
    LAUNCH_PACK_BPE_MR(k_pack_mlm_bpe_flush);
    return hipGetLastError();
}
#undef LAUNCH_PACK_BPE_MR
#undef LAUNCH_PACK_BPE

}  // namespace sdl
