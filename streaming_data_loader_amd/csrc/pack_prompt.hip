// pack_prompt.hip -- packed CLM rows over prompt / completion examples with completion-only labels
// (sdl_config.pair = 6, SDL_PAIR_CLM_COMPLETION, on a pack = 1 handle; DESIGN.md §3 "Prompt /
// completion rows") on gfx950.
//
// A call's 2 E text ranges are E examples: range 2e is the prompt A_e, range 2e + 1 the completion
// B_e, tokenized as records of their own.  A kept example enters pack.hip's stream as the document
//     a_e ++ b_e ++ [eos]                                                  nA + nB + 1
// and the planes are the plain packed ones over these documents but for labels, which is -100 on
// every id of some a_e.  The geometry is k_pack_gather's (1024 positions a wave in rounds of 64
// groups of four, one wave-uniform binary search a wave -- over E examples, not 2 E ranges -- lanes
// walking on from their last example, whole 16-byte non-temporal stores).
//
// The id map is the plain one.  k_records gives every range q the ids [T(q), T(q + 1)) of the dense
// array with one function T of the range's first text byte (rec_tok[q] = T(q), rec_cnt[q] =
// T(q + 1) - T(q)), so  rec_tok[2e + 1] == rec_tok[2e] + rec_cnt[2e]  for every range: an empty
// one (T(q) == T(q + 1)), one whose long pieces k_bpe_long finished (they are counted in the chunk
// scan T is made of) and one with a tokenize error (its ids may be short, the partition is not).
// A document's ids are tok[rec_tok[2e] .. + nA + nB), the seam is a count, and a group needs the
// pair {nA, nB} (one 8-byte load) and rec_tok[2e] -- no plan buffer, no third dependent load.
//
// The carry keeps, beside pack.hip's ids and position_ids, a flag per position (1: a prompt id) in
// a buffer of this feature's own, so a call that ends inside a prompt continues with -100 labels
// and the flush row has them too; k_pack_flush knows no flags, hence k_prompt_flush.
#include "device_util.hpp"
#include "kernels.hpp"
#include "pack_search.hpp"

namespace sdl {

// {nA, nB} of example e: rec_cnt[2e], rec_cnt[2e + 1] as one 8-byte load (rec_cnt is a device
// allocation, 2e is even)
__device__ __forceinline__ uint2 prompt_counts(const PackPromptParams &q, uint32_t e) {
    return reinterpret_cast<const uint2 *>(q.rec_cnt)[e];
}

// Per example: its packed length (nA + nB + 1, or 0 when dropped: no completion id, or below
// min_ids) into rec_len (sdl_device_rows.d_record_rows, E entries); thread 0 seeds the scan with the
// carry length.
__global__ __launch_bounds__(256) void k_prompt_lengths(PackPromptParams q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) q.pk_off[0] = *q.carry_len;
    for (int64_t e = i; e < q.E; e += (int64_t)gridDim.x * 256) {
        const uint2 c = prompt_counts(q, (uint32_t)e);
        const uint32_t n = c.x + c.y + 1u;
        q.rec_len[e] = c.y >= 1u && n >= (uint32_t)(q.min_ids > 0 ? q.min_ids : 0) ? n : 0u;
    }
}

// The id and label at index i (0 <= i <= nA + nB) of a kept example (nB >= 1) whose ids start at
// tok[base]: the load is issued for every i at a clamped address and the eos selected afterwards,
// so the loads of a group do not wait for one another.
__device__ __forceinline__ void prompt_id(const PackPromptParams &q, uint32_t base, uint2 c, uint32_t i, int32_t &id,
                                          int32_t &lab) {
    const uint32_t n = c.x + c.y;
    const int32_t t = (int32_t)q.tok[base + (i < n ? i : n - 1u)];
    id = i >= n ? q.eos : t;
    lab = i < c.x ? -100 : id;
}

struct PromptElem {
    int32_t id, lab, pos;
};
// Stream position p (c0 <= p < L) of example e: its id, label and position_id.
__device__ __forceinline__ PromptElem prompt_elem(const PackPromptParams &q, uint32_t e, uint32_t p, uint32_t start) {
    const uint32_t row0 = p / (uint32_t)q.S * (uint32_t)q.S;
    PromptElem x;
    prompt_id(q, q.rec_tok[2u * e], prompt_counts(q, e), p - start, x.id, x.lab);
    x.pos = (int32_t)(p - (start > row0 ? start : row0));
    return x;
}

__device__ __forceinline__ void prompt_store4(int32_t *__restrict__ o, uint32_t p, uint32_t end, const int32_t (&v)[4]) {
    if (p + 4u <= end) {  // the planes stream out: non-temporal, this pass does not read them again
        typedef int32_t v4i __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(v4i{v[0], v[1], v[2], v[3]}, reinterpret_cast<v4i *>(o + p));
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (p + (uint32_t)w < end) o[p + w] = v[w];
    }
}

// The four planes over the flat output index, in k_pack_gather's geometry.  A group of four
// positions inside one example and below the stream's last full row loads the example's counts and
// first id once and issues its four id loads independently -- also when the A/B seam, the eos or a
// row end lies inside the group; a group that crosses an example's end, the carry or the stream's
// end takes the chained loop.
constexpr uint32_t PROMPT_WAVE_POS = 1024u;
constexpr uint32_t PROMPT_TILE = 4u * PROMPT_WAVE_POS;
__global__ __launch_bounds__(256) void k_prompt_gather(PackPromptParams q) {
    const uint32_t S = (uint32_t)q.S, E = (uint32_t)q.E;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[E];
    const uint32_t G = L / S, full = G * S;
    uint64_t gpad = ((uint64_t)G + (uint64_t)q.B - 1u) / (uint64_t)q.B * (uint64_t)q.B;
    if (gpad > (uint64_t)q.rows_cap) gpad = (uint64_t)q.rows_cap;
    const uint32_t end = (uint32_t)(gpad * S);  // (rows_cap * S < 2^32: checked by the host)
    const int lane = lane_id();
    for (uint64_t t0 = (uint64_t)blockIdx.x * PROMPT_TILE; t0 < end; t0 += (uint64_t)gridDim.x * PROMPT_TILE) {
        const uint32_t wb = (uint32_t)t0 + (uint32_t)(threadIdx.x >> 6) * PROMPT_WAVE_POS;  // the wave's first position
        if (wb >= end) continue;
        // wave-uniform: the example of the wave's first stream position past the carry (when it has one)
        uint32_t e = 0;
        const uint32_t wf = wb > c0 ? wb : c0;
        if (wf < full) e = pack_record_of(q.pk_off, 0u, E - 1u, wf);  // (full > c0: E > 0)
        for (uint32_t k = 0; k < PROMPT_WAVE_POS / 256u; ++k) {
            const uint32_t p0 = wb + 256u * k + 4u * (uint32_t)lane;
            if (p0 >= end) break;
            int32_t id[4], am[4], lab[4], pos[4];
            if (p0 >= full) {  // padding rows only
#pragma unroll
                for (int w = 0; w < 4; ++w) id[w] = 0, am[w] = 1, lab[w] = -100, pos[w] = 0;
            } else {
                uint32_t start = 0, next = 0;
                const uint32_t pf = p0 > c0 ? p0 : c0;  // the lane's first position past the carry
                if (pf < full) {  // (pf >= wf, and pk_off[e] <= the lane's last position: e is at or below pf's example)
                    e = pack_record_near(q.pk_off, e, E - 1u, pf);
                    start = q.pk_off[e];
                    next = q.pk_off[e + 1u];
                }
                if (p0 >= c0 && p0 + 3u < next && p0 + 3u < full) {
                    const uint2 c = prompt_counts(q, e);
                    const uint32_t base = q.rec_tok[2u * e], i0 = p0 - start;
                    const uint32_t row0 = p0 / S * S;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const uint32_t p = p0 + (uint32_t)w;
                        const uint32_t rs = p - row0 < S ? row0 : p / S * S;  // (a row end inside the group)
                        prompt_id(q, base, c, i0 + (uint32_t)w, id[w], lab[w]);
                        pos[w] = (int32_t)(p - (start > rs ? start : rs));
                        am[w] = 1;
                    }
                } else {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const uint32_t p = p0 + (uint32_t)w;
                        if (p >= full) {
                            id[w] = 0, am[w] = 1, lab[w] = -100, pos[w] = 0;
                        } else if (p < c0) {  // (the carry lies in row 0)
                            id[w] = q.carry_ids[p];
                            lab[w] = q.carry_flag[p] ? -100 : id[w];
                            pos[w] = q.carry_pos[p];
                            am[w] = 1;
                        } else {
                            while (p >= next) {  // p < L = pk_off[E]: ends at an example of length > 0
                                ++e;
                                start = next;
                                next = q.pk_off[e + 1u];
                            }
                            const PromptElem x = prompt_elem(q, e, p, start);
                            id[w] = x.id;
                            lab[w] = x.lab;
                            pos[w] = x.pos;
                            am[w] = 1;
                        }
                    }
                }
            }
            prompt_store4(q.ids, p0, end, id);
            prompt_store4(q.am, p0, end, am);
            prompt_store4(q.lab, p0, end, lab);
            prompt_store4(q.pos, p0, end, pos);
        }
    }
}

// stream[G S :), its position_ids in the row it will open and its prompt flags -> the other half of
// the carry, through the same element map; the new length and the call's row count (one workgroup;
// fewer than S <= 4096 elements).
__global__ __launch_bounds__(256) void k_prompt_carry(PackPromptParams q) {
    const uint32_t S = (uint32_t)q.S, E = (uint32_t)q.E;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[E];
    const uint32_t G = L / S, full = G * S, n = L - full;
    for (uint32_t x = threadIdx.x; x < n; x += 256u) {
        const uint32_t p = full + x;
        if (p < c0) {  // (G == 0: the old carry stays in front)
            q.new_ids[x] = q.carry_ids[p];
            q.new_pos[x] = q.carry_pos[p];
            q.new_flag[x] = q.carry_flag[p];
        } else {
            const uint32_t e = pack_record_of(q.pk_off, 0u, E - 1u, p);  // (p >= c0 and p < L: E > 0)
            const PromptElem v = prompt_elem(q, e, p, q.pk_off[e]);
            q.new_ids[x] = v.id;
            q.new_pos[x] = v.pos;
            q.new_flag[x] = v.lab == -100 ? 1u : 0u;  // (no id is negative)
        }
    }
    if (threadIdx.x == 0) {
        *q.new_len = n;
        *q.d_rows = G;
    }
}

// The flush row: k_pack_flush's, with labels -100 on the carry's prompt positions as well as behind
// the carry; rows 1 .. B - 1 get the padding rows' initial values; the other half's length becomes
// 0.  c == 0 emits no row.
__global__ __launch_bounds__(256) void k_prompt_flush(PackPromptParams q) {
    const uint32_t S = (uint32_t)q.S, c = *q.carry_len;
    uint64_t rows = (uint64_t)q.B;
    if (rows > (uint64_t)q.rows_cap) rows = (uint64_t)q.rows_cap;
    const uint64_t end = rows * S;
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < end; p += (uint64_t)gridDim.x * 256u) {
        int32_t id = 0, am = 1, lab = -100, pos = 0;
        if (p < S && c > 0u) {
            am = 0;
            if (p < c) {
                id = q.carry_ids[p];
                lab = q.carry_flag[p] ? -100 : id;
                pos = q.carry_pos[p];
                am = 1;
            }
        }
        q.ids[p] = id;
        q.am[p] = am;
        q.lab[p] = lab;
        q.pos[p] = pos;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *q.new_len = 0u;
        *q.d_rows = c > 0u ? 1u : 0u;
    }
}

hipError_t launch_prompt_lengths(const PackPromptParams &q, hipStream_t st) {
    const int64_t want = (q.E + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 1024 ? want : 1024);
    hipLaunchKernelGGL(k_prompt_lengths, dim3(grid), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t launch_prompt_rows(const PackPromptParams &q, hipStream_t st) {
    const int64_t tiles = (q.rows_cap * q.S + (int64_t)PROMPT_TILE - 1) / (int64_t)PROMPT_TILE;
    const unsigned grid = (unsigned)(tiles < 1 ? 1 : tiles < 16384 ? tiles : 16384);
    hipLaunchKernelGGL(k_prompt_gather, dim3(grid), dim3(256), 0, st, q);
    hipLaunchKernelGGL(k_prompt_carry, dim3(1), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t launch_prompt_flush(const PackPromptParams &q, hipStream_t st) {
    const int64_t want = ((int64_t)q.B * q.S + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 4096 ? want : 4096);
    hipLaunchKernelGGL(k_prompt_flush, dim3(grid), dim3(256), 0, st, q);
    return hipGetLastError();
}

}  // namespace sdl
