// pair_mlm.hip -- BERT / ALBERT pre-training rows on gfx950: one [CLS] A [SEP] B [SEP] row per
// example of two texts with a BERT masking policy applied and a sentence-level label drawn
// (sdl_config.pair 2..4, DESIGN.md §3 "Sentence pairs").
//
// The tokenizer ran over the call's 2 * n_pairs text ranges and launch_records left each range's
// first id and id count, as for k_rows_pair (pair.hip).  A row here is a function of one Philox
// block -- the draw that says which two ranges are its segments (pair_draw.hpp: the pair's own, a
// foreign second segment under NSP, the two swapped under SOP) -- and of the four words rec_tok /
// rec_cnt of the chosen ranges: the kept lengths are tokenizers' longest_first truncation of the
// chosen sides, every position's source follows from five boundaries, and the ids are read from
// the WordPiece chunk lists themselves (list_index.hpp), no dense copy.  The masking is the policy
// contract of the unpaired rows (rows_device.hpp row_policy_one) applied to that row as chunk 0 of
// record first_record + r: the same keys, units, pick and 80/10/10 replacement, with the pair row's
// l = k_a + k_b + 3 filled positions, token types and plain attention mask.
//
// Geometry: k_rows_policy's -- a wave per row, four rows a block, lane L owns positions
// 256 m + 4 L + w of its row, MR rounds of them; the whole-word build has the wave's 256 MR words
// of LDS.  One launch writes the four planes of every row up to the next multiple of B, the pair
// label of each and the one-segment row tables (row_off, row_rec, rb) that the host path reads.
#include "device_util.hpp"
#include "kernels.hpp"
#include "pair_draw.hpp"
#include "rows_device.hpp"

namespace sdl {

template <int MR, bool WHOLE>
__device__ __forceinline__ void row_pair_mlm_one(const PairMlmParams &q, uint32_t g, uint32_t G, uint32_t *lds,
                                                 int lane) {
    const int S = q.S;
    const bool vec = (S & 3) == 0;
    int32_t *ids_o = q.ids + (size_t)g * S;
    int32_t *am_o = q.am + (size_t)g * S;
    int32_t *tt_o = q.tt + (size_t)g * S;
    int32_t *lb_o = q.lab + (size_t)g * S;
    if (g >= G) {  // rows of the last batch nobody filled: the unpaired mlm initial values
#pragma unroll
        for (int m = 0; m < MR; ++m) {
            const int j0 = 256 * m + 4 * lane;
            store4(ids_o, j0, S, vec, 0, 0, 0, 0);
            store4(am_o, j0, S, vec, 1, 1, 1, 1);
            store4(tt_o, j0, S, vec, 0, 0, 0, 0);
            store4(lb_o, j0, S, vec, -100, -100, -100, -100);
        }
        if (lane == 0) q.pair_lab[g] = -100;
        return;
    }
    // the draw, the two chosen text ranges and their kept lengths
    const uint64_t rec = q.first_record + (uint64_t)g;
    const PairDraw d = pair_draw(q.seed, rec, g, G, q.mode);
    const uint32_t ta = q.rec_tok[d.first], tb = q.rec_tok[d.second];
    const PairKeptLengths k = pair_kept_lengths(q.rec_cnt[d.first], q.rec_cnt[d.second], (uint32_t)S - 3u);
    // the chunks each side's ids lie in (those of its own bytes); a lane's ids have rising
    // indices, so each search starts at the chunk of the one before
    ListBracket ba = list_bracket(q.off[d.first], q.off[d.first + 1u], q.n_lists);
    ListBracket bb = list_bracket(q.off[d.second], q.off[d.second + 1u], q.n_lists);
    // columns: [CLS] at 0, a at [1, c1), [SEP] at c1, b at [c2, c3), [SEP] at c3, padding from c4
    const uint32_t c1 = 1u + k.a, c2 = c1 + 1u, c3 = c2 + k.b, c4 = c3 + 1u;
    const int l = (int)c4;  // filled positions (<= S)
    if (lane == 0) {
        q.pair_lab[g] = d.label;
        q.row_off[g] = g;
        q.row_rec[g] = g;
    }
    int32_t id[MR][4];
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t j = (uint32_t)(256 * m + 4 * lane + w);
            const bool in_a = j >= 1u && j < c1, in_b = j >= c2 && j < c3;
            int32_t v = 0;
            if (in_a) {  // (k_a >= 1: the side has bytes, so n_lists >= 1 and the bracket is valid)
                const uint32_t ti = ta + (j - 1u);
                ba.lo = list_chunk_of(q.chunk_off, ba.lo, ba.hi, ti);
                v = (int32_t)q.lists[list_slot(q.chunk_off, ba.lo, ti)];
            }
            if (in_b) {
                const uint32_t ti = tb + (j - c2);
                bb.lo = list_chunk_of(q.chunk_off, bb.lo, bb.hi, ti);
                v = (int32_t)q.lists[list_slot(q.chunk_off, bb.lo, ti)];
            }
            if (j == 0u) v = q.cls;
            if (j == c1 || j == c3) v = q.sep;
            id[m][w] = v;
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
    int kb = (int)(((int64_t)l * mp.per_mille + 500) / 1000);
    kb = kb < 1 ? 1 : kb;
    kb = kb < q.mask_length ? kb : q.mask_length;
    if (ncand == 0) kb = 0;

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
    // the lanes that own a picked position; then the four planes
#pragma unroll
    for (int m = 0; m < MR; ++m) {
        const int j0 = 256 * m + 4 * lane;
        const uint32_t s4 = (sel >> (4 * m)) & 15u;
        int32_t v[4], lab[4], am[4], tt[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t j = (uint32_t)(j0 + w);
            v[w] = id[m][w];
            lab[w] = -100;
            am[w] = j < c4 ? 1 : 0;
            tt[w] = j >= c2 && j < c4 ? 1 : 0;
        }
        if (s4) {
            const uint4 u4 = philox4x32_10(make_uint4((uint32_t)(64 * m + lane), 0x20000000u, (uint32_t)rec,
                                                      (uint32_t)(rec >> 32)),
                                           (uint32_t)q.seed, (uint32_t)(q.seed >> 32));
            const uint32_t u[4] = {u4.x, u4.y, u4.z, u4.w};
            bool any_rand = false;
#pragma unroll
            for (int w = 0; w < 4; ++w)
                any_rand = any_rand || ((s4 >> w) & 1u && u[w] >= 0xCCCCCCCDu && u[w] < 0xE6666667u);
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
                    if (u[w] < 0xCCCCCCCDu) v[w] = q.mask_id;
                    else if (u[w] < 0xE6666667u) v[w] = (int32_t)__umulhi(rr[w], mp.vocab_size);
                }
        }
        store4(ids_o, j0, S, vec, v[0], v[1], v[2], v[3]);
        store4(am_o, j0, S, vec, am[0], am[1], am[2], am[3]);
        store4(tt_o, j0, S, vec, tt[0], tt[1], tt[2], tt[3]);
        store4(lb_o, j0, S, vec, lab[0], lab[1], lab[2], lab[3]);
    }
}

template <int MR, bool WHOLE>
__global__ __launch_bounds__(256) void k_rows_pair_mlm(PairMlmParams q) {
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ uint32_t s_unit[WHOLE ? 4 : 1][WHOLE ? 256 * MR : 1];
    const uint32_t G = (uint32_t)q.n_pairs, g_end = (uint32_t)q.rows_end;
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // one segment, a row per pair
        q.rb[0] = 0u;
        q.rb[1] = G;
        q.row_off[G] = G;
    }
    for (uint32_t g = blockIdx.x * 4u + (uint32_t)wid; g < g_end; g += gridDim.x * 4u)
        row_pair_mlm_one<MR, WHOLE>(q, g, G, s_unit[WHOLE ? wid : 0], lane);
}

hipError_t launch_rows_pair_mlm(const PairMlmParams &q, hipStream_t st) {
    if (q.S < 3 || q.S > 2048 || q.n_pairs < 0 || q.n_pairs >= ((int64_t)1 << 31) || q.rows_end < q.n_pairs ||
        q.rows_end * (int64_t)q.S >= ((int64_t)1 << 32) || q.mode < PAIR_MODE_MLM || q.mode > PAIR_MODE_MLM_SOP ||
        q.mp.policy < 1 || q.mp.policy > 2 || (q.mp.policy == 2 && !q.mp.cont_bits) || !q.lab || !q.tt || !q.pair_lab)
        return hipErrorInvalidValue;
    const int64_t want = (q.rows_end + 3) / 4;  // (a call of no pairs still writes rb and row_off[0])
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 16384 ? want : 16384);
    const int MR = (q.S + 255) / 256;
#define LAUNCH_PAIR_MLM(MM)                                                                                  \
    do {                                                                                                     \
        if (q.mp.policy == 2) hipLaunchKernelGGL((k_rows_pair_mlm<MM, true>), dim3(grid), dim3(256), 0, st, q); \
        else hipLaunchKernelGGL((k_rows_pair_mlm<MM, false>), dim3(grid), dim3(256), 0, st, q);               \
    } while (0)
    if (MR <= 1) LAUNCH_PAIR_MLM(1);
    else if (MR <= 2) LAUNCH_PAIR_MLM(2);
    else if (MR <= 4) LAUNCH_PAIR_MLM(4);
    else LAUNCH_PAIR_MLM(8);
#undef LAUNCH_PAIR_MLM
    return hipGetLastError();
}

}  // namespace sdl
