// pack_mlm.hip -- MLM rows packed from the concatenated document stream with a BERT masking policy
// applied to every row (sdl_config.pack = 1 under the MLM task, DESIGN.md §3 "Packed rows") on
// gfx950: HF run_mlm.py's group_texts / RoBERTa's FULL-SENTENCES.
//
// The call's stream is  carry ++ concat over kept records r of ([CLS] ++ ids_r ++ [SEP]),  pk_off[r]
// the stream position where record r starts (pack.hip's scan, with two framing ids a record), and
// row g of the call is stream[g S, (g + 1) S).  pack.hip gathers over the flat output index from a
// dense id array and cannot mask -- a mask is a selection over one row; k_rows_policy masks a row of
// one record.  Here a wave owns one packed row: it finds the record of the row's first position by
// one wave-uniform binary search in pk_off, every lane walks forward from there to the records of
// its own columns (a galloping search per round of 256 columns, single steps inside a group of
// four), and the ids are read from the WordPiece chunk lists themselves (list_index.hpp: the
// chunks of the record's bytes, each search continuing from the lane's last chunk) -- no dense
// copy of the ids.  With the row in registers the wave runs the policy contract of the unpacked
// rows (rows_device.hpp row_policy_one) on it as chunk 0 of record q, the row's packed index on the
// handle: the same keys, units, pick and 80/10/10 replacement, l = S filled positions.
//
// Geometry: k_rows_policy's -- four rows a block, lane L owns columns 256 m + 4 L + w of its row,
// MR rounds of them; the whole-word build has the wave's 256 MR words of LDS.  A document's end is
// a record's end (pk_off), never an id compared with [SEP]; the carry keeps its position_ids
// beside its (unmasked) ids for the same reason.
#include "device_util.hpp"
#include "kernels.hpp"
#include "pack_search.hpp"
#include "rows_device.hpp"

#ifndef SDL_PACK_MLM_ABLATE  // build.py build_pack_mlm_ablations: where the rows kernel spends its time
#define SDL_PACK_MLM_ABLATE 0
#endif

namespace sdl {

// A lane's place in the stream: the record of its last position, that record's extent, and (once
// `known`) its id count, first id and the chunks its ids lie in.  Positions only rise.
struct PackCursor {
    uint32_t r, start, next;
    uint32_t n, base;
    ListBracket br;
    uint32_t cb, cn;  // the ids of chunk br.lo: [cb, cb + cn) (cn = 0: not loaded)
    bool known;
};

__device__ __forceinline__ PackCursor pack_cursor(const PackMlmParams &q, uint32_t r) {
    PackCursor c;
    c.r = r;
    c.start = q.pk_off[r];
    c.next = q.pk_off[r + 1u];
    c.n = c.base = c.cb = c.cn = 0u;
    c.br = ListBracket{0, 0};
    c.known = false;
    return c;
}

struct PackMlmElem {
    int32_t id, pos;
};
// Stream position p (c0 <= p < L, at or past the cursor's record start) in the row that starts at
// row0: its unmasked id and position_id.  far: the record may lie many records on (a lane's next
// round) -- gallop; else step (runs of dropped records share an offset and are stepped over).
__device__ __forceinline__ PackMlmElem pack_mlm_elem(const PackMlmParams &q, PackCursor &c, uint32_t p, uint32_t row0,
                                                     bool far) {
    if (p >= c.next) {
        uint32_t r = far ? pack_record_near(q.pk_off, c.r, (uint32_t)q.R - 1u, p) : c.r;
        uint32_t start = q.pk_off[r], next = q.pk_off[r + 1u];
        while (p >= next) {  // p < L = pk_off[R]: ends at a record of length > 0
            ++r;
            start = next;
            next = q.pk_off[r + 1u];
        }
        c.r = r;
        c.start = start;
        c.next = next;
        c.known = false;
    }
    if (!c.known) {  // (a kept record has ids, so bytes: n_lists >= 1 and the bracket is valid)
        c.n = q.rec_cnt[c.r];
        c.base = q.rec_tok[c.r];
        c.br = list_bracket(q.off[c.r], q.off[c.r + 1u], q.n_lists);
        c.cb = c.cn = 0u;
        c.known = true;
    }
    const uint32_t i = p - c.start;  // the document is [CLS] ids [SEP]
    PackMlmElem e;
    if (i == 0u) {
        e.id = q.cls;
    } else if (i > c.n) {
        e.id = q.sep;
    } else {
        const uint32_t ti = c.base + i - 1u;
#if SDL_PACK_MLM_ABLATE >= 2  // (diagnostic: no chunk search, no list read; the rows are not the contract's)
        e.id = 1000 + (int32_t)(ti & 1023u);
#else
        if (ti - c.cb >= c.cn) {  // not in the lane's last chunk (ids [cb, cb + cn)): search on from it
            c.br.lo = list_chunk_of(q.chunk_off, c.br.lo, c.br.hi, ti);
            c.cb = q.chunk_off[c.br.lo];
            c.cn = q.chunk_off[c.br.lo + 1] - c.cb;
        }
        e.id = (int32_t)q.lists[c.br.lo * LIST_STRIDE + (int64_t)(ti - c.cb)];  // (list_slot, chunk_off[lo] held)
#endif
    }
    e.pos = (int32_t)(p - (c.start > row0 ? c.start : row0));
    return e;
}

// A row nobody filled: the unpacked mlm initial values, position_ids 0.
template <int MR>
__device__ __forceinline__ void pack_mlm_pad_row(const PackMlmParams &q, uint32_t g, int lane) {
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
// carry), masked as chunk 0 of record `rec`; columns >= l: ids 0, attention 0, labels -100.
template <int MR, bool WHOLE>
__device__ __forceinline__ void pack_mlm_row(const PackMlmParams &q, uint32_t g, uint32_t row0, int l, uint32_t c0,
                                             uint64_t rec, uint32_t *lds, int lane) {
    const int S = q.S;
    const bool vec = (S & 3) == 0;
    int32_t *ids_o = q.ids + (size_t)g * S;
    int32_t *am_o = q.am + (size_t)g * S;
    int32_t *tt_o = q.tt + (size_t)g * S;
    int32_t *lb_o = q.lab + (size_t)g * S;
    int32_t *ps_o = q.pos + (size_t)g * S;
    // the record of the row's first position past the carry, once a wave
    PackCursor cur{};
    const uint32_t wf = row0 > c0 ? row0 : c0;
    if (wf < row0 + (uint32_t)l)  // (then R > 0 and wf < L)
        cur = pack_cursor(q, (uint32_t)__builtin_amdgcn_readfirstlane(
                                 (int)pack_record_of(q.pk_off, 0u, (uint32_t)q.R - 1u, wf)));
    int32_t id[MR][4];
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        const int j0 = 256 * m + 4 * lane;
        int32_t ps[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int j = j0 + w;
            int32_t v = 0, pp = 0;
            if (j < l) {
                const uint32_t p = row0 + (uint32_t)j;
                if (p < c0) {  // (the carry lies in row 0)
                    v = q.carry_ids[p];
                    pp = q.carry_pos[p];
                } else {
                    const PackMlmElem e = pack_mlm_elem(q, cur, p, row0, w == 0);
                    v = e.id;
                    pp = e.pos;
                }
            }
            id[m][w] = v;
            ps[w] = pp;
        }
        store4(ps_o, j0, S, vec, ps[0], ps[1], ps[2], ps[3]);
        store4(tt_o, j0, S, vec, 0, 0, 0, 0);
    }
    const MaskPolicy &mp = q.mp;
    const PickWave wv{(uint32_t)lane};

    // candidates: filled positions whose id is none of 0, mask_id, [CLS] and [SEP]
    uint32_t cand = 0;
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int32_t v = id[m][w];
            const bool ex = v == 0 || v == q.mask_id || v == q.cls || v == q.sep;
            if (256 * m + 4 * lane + w < l && !ex) cand |= 1u << (4 * m + w);
        }
    const int ncand = (int)wv.sum((uint32_t)__popc(cand));
    int kb = policy_budget(l, ncand, mp.per_mille, q.mask_length);
#if SDL_PACK_MLM_ABLATE >= 1  // (diagnostic: no keys, no pick, no draws; the rows are not the contract's)
    kb = 0;
#endif

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
            auto step = [] {  // one lane's LDS writes before the others' reads (a wave: program order)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            };
            // continuation bits of the candidates' ids
            uint32_t cont = 0;
#pragma unroll
            for (int e = 0; e < 4 * MR; ++e) {
                const uint32_t v = (uint32_t)id[e >> 2][e & 3];
                const uint32_t wd = (cand >> e) & 1u && v < mp.vocab_size ? mp.cont_bits[v >> 5] : 0u;
                cont |= ((wd >> (v & 31u)) & 1u) << e;
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
                    else if (u[w] < POLICY_RANDOM_BELOW) v[w] = (int32_t)__umulhi(rr[w], mp.vocab_size);
                }
        }
        store4(ids_o, j0, S, vec, v[0], v[1], v[2], v[3]);
        store4(am_o, j0, S, vec, am[0], am[1], am[2], am[3]);
        store4(lb_o, j0, S, vec, lab[0], lab[1], lab[2], lab[3]);
    }
}

// The five planes of the call's rows: rows [0, G) the stream, [G, end) the padding rows up to the
// next multiple of B.  The grid is sized from the upper bound rows_cap -- the row count stays on
// the device -- and the packed index of row g is the handle's counter (the half the last call
// wrote; k_pack_mlm_carry writes the other one) plus g.
template <int MR, bool WHOLE>
__global__ __launch_bounds__(256) void k_pack_mlm_rows(PackMlmParams q) {
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ uint32_t s_unit[WHOLE ? 4 : 1][WHOLE ? 256 * MR : 1];
    const uint32_t S = (uint32_t)q.S, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / S;
    uint64_t gpad = ((uint64_t)G + (uint64_t)q.B - 1u) / (uint64_t)q.B * (uint64_t)q.B;
    if (gpad > (uint64_t)q.rows_cap) gpad = (uint64_t)q.rows_cap;
    const uint32_t end = (uint32_t)gpad;  // (rows_cap * S < 2^32: checked by the host)
    const uint64_t q0 = *q.row_cnt;
    for (uint32_t g = blockIdx.x * 4u + (uint32_t)wid; g < end; g += gridDim.x * 4u) {
        if (g < G) pack_mlm_row<MR, WHOLE>(q, g, g * S, (int)S, c0, q0 + g, s_unit[WHOLE ? wid : 0], lane);
        else pack_mlm_pad_row<MR>(q, g, lane);
    }
}

// stream[G S :) unmasked, with its position_ids in the row it will open -> the other half of the
// carry, the new length, the row counter advanced by G and the call's row count (one workgroup;
// fewer than S <= 2048 elements).
__global__ __launch_bounds__(256) void k_pack_mlm_carry(PackMlmParams q) {
    const uint32_t S = (uint32_t)q.S, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / S, full = G * S, n = L - full;
    for (uint32_t x = threadIdx.x; x < n; x += 256u) {
        const uint32_t p = full + x;
        if (p < c0) {  // (G == 0: the old carry stays in front)
            q.new_ids[x] = q.carry_ids[p];
            q.new_pos[x] = q.carry_pos[p];
        } else {
            PackCursor cur = pack_cursor(q, pack_record_of(q.pk_off, 0u, R - 1u, p));
            const PackMlmElem e = pack_mlm_elem(q, cur, p, full, false);
            q.new_ids[x] = e.id;
            q.new_pos[x] = e.pos;
        }
    }
    if (threadIdx.x == 0) {
        *q.new_len = n;
        *q.new_row_cnt = *q.row_cnt + G;
        *q.d_rows = G;
    }
}

// The flush row: the carry's c ids in row 0, masked with l = c and the next packed index, the plain
// orientation past them; rows 1 .. B - 1 (and row 0 when c == 0) get the padding rows' initial
// values; the other half's length becomes 0 and its counter the old one plus the row.
template <int MR, bool WHOLE>
__global__ __launch_bounds__(256) void k_pack_mlm_flush(PackMlmParams q) {
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ uint32_t s_unit[WHOLE ? 4 : 1][WHOLE ? 256 * MR : 1];
    const uint32_t c = *q.carry_len;
    const uint64_t q0 = *q.row_cnt;
    const uint32_t end = (uint32_t)((int64_t)q.B < q.rows_cap ? (int64_t)q.B : q.rows_cap);
    for (uint32_t g = blockIdx.x * 4u + (uint32_t)wid; g < end; g += gridDim.x * 4u) {
        if (g == 0u && c > 0u) pack_mlm_row<MR, WHOLE>(q, 0u, 0u, (int)c, c, q0, s_unit[WHOLE ? wid : 0], lane);
        else pack_mlm_pad_row<MR>(q, g, lane);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *q.new_len = 0u;
        *q.new_row_cnt = q0 + (c > 0u ? 1u : 0u);
        *q.d_rows = c > 0u ? 1u : 0u;
    }
}

static bool pack_mlm_ok(const PackMlmParams &q) {
    return q.S >= 3 && q.S <= 2048 && q.B > 0 && q.R >= 0 && q.R < ((int64_t)1 << 32) - 1 && q.rows_cap >= 0 &&
           q.rows_cap * (int64_t)q.S < ((int64_t)1 << 32) && q.mp.policy >= 1 && q.mp.policy <= 2 &&
           (q.mp.policy != 2 || q.mp.cont_bits) && q.ids && q.am && q.tt && q.lab && q.pos;
}

#define LAUNCH_PACK_MLM(KERNEL, MM)                                                                  \
    do {                                                                                             \
        if (q.mp.policy == 2) hipLaunchKernelGGL((KERNEL<MM, true>), dim3(grid), dim3(256), 0, st, q); \
        else hipLaunchKernelGGL((KERNEL<MM, false>), dim3(grid), dim3(256), 0, st, q);                \
    } while (0)
#define LAUNCH_PACK_MLM_MR(KERNEL)             \
    do {                                       \
        const int MR = (q.S + 255) / 256;      \
        if (MR <= 1) LAUNCH_PACK_MLM(KERNEL, 1); \
        else if (MR <= 2) LAUNCH_PACK_MLM(KERNEL, 2); \
        else if (MR <= 4) LAUNCH_PACK_MLM(KERNEL, 4); \
        else LAUNCH_PACK_MLM(KERNEL, 8);         \
    } while (0)

hipError_t launch_pack_mlm_rows(const PackMlmParams &q, hipStream_t st) {
    if (!pack_mlm_ok(q)) return hipErrorInvalidValue;
    const int64_t want = (q.rows_cap + 3) / 4;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 16384 ? want : 16384);
    LAUNCH_PACK_MLM_MR(k_pack_mlm_rows);
    hipLaunchKernelGGL(k_pack_mlm_carry, dim3(1), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t launch_pack_mlm_flush(const PackMlmParams &q, hipStream_t st) {
    if (!pack_mlm_ok(q)) return hipErrorInvalidValue;
    const int64_t want = ((int64_t)q.B + 3) / 4;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 4096 ? want : 4096);
    LAUNCH_PACK_MLM_MR(k_pack_mlm_flush);
    return hipGetLastError();
}
#undef LAUNCH_PACK_MLM_MR
#undef LAUNCH_PACK_MLM

}  // namespace sdl
