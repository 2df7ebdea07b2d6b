// pack_fim.hip -- packed CLM rows with fill-in-the-middle documents (sdl_batcher_set_fim on a
// pack = 1 handle, DESIGN.md §3 "Fill-in-the-middle") on gfx950.
//
// pack.hip's stream, but a drawn share of the documents enters it permuted: with t the n ids of a
// record and cuts a <= b,
//     untouched   t ++ [eos]                                                       n + 1
//     PSM         [PRE] ++ t[0:a] ++ [SUF] ++ t[b:n] ++ [MID] ++ t[a:b] ++ [eos]   n + 4
//     SPM         [PRE, SUF] ++ t[b:n] ++ [MID] ++ t[0:b] ++ [eos]                 n + 4
// No transformed copy of the ids exists: k_fim_plan draws one Philox block a record and leaves an
// 8-byte plan word (a, b, two flags) beside the record's stream length, the lengths are scanned
// into pk_off as for the plain rows, and the gather over the flat output index reads every id from
// the dense array through the plan -- a document is at most three runs of consecutive source ids
// with a constant offset each (FimMap), so a position costs two compares and an add on top of the
// plain gather.  The geometry is k_pack_gather's (1024 positions a wave in rounds of 64 groups of
// four, one wave-uniform binary search a wave, lanes walking on from their last record, whole
// 16-byte non-temporal stores), and the flush kernel is pack.hip's: the carry holds transformed ids.
#include "device_util.hpp"
#include "kernels.hpp"
#include "mlm_policy_device.hpp"
#include "pack_search.hpp"

namespace sdl {

// Per record: the draw (kept records only, counter (0, FIM_DOMAIN, d lo, d hi) with d = first_record
// + records the handle saw before + r), the plan word and the stream length into rec_len
// (sdl_device_rows.d_record_rows); thread 0 seeds the scan with the carry length.
__global__ __launch_bounds__(256) void k_fim_plan(PackFimParams q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) q.pk_off[0] = *q.carry_len;
    const uint64_t d0 = q.first_record + *q.rec_seen;
    const uint64_t rate = (uint64_t)q.rate << 32, spm = (uint64_t)q.spm << 32;
    for (int64_t r = i; r < q.R; r += (int64_t)gridDim.x * 256) {
        const uint32_t n = q.rec_cnt[r];
        const bool keep = n >= 1u && n + 1u >= (uint32_t)(q.min_ids > 0 ? q.min_ids : 0);
        uint2 plan = make_uint2(0u, 0u);
        if (keep && q.rate > 0) {
            const uint64_t d = d0 + (uint64_t)r;
            const uint4 x = philox4x32_10(make_uint4(0u, FIM_DOMAIN, (uint32_t)d, (uint32_t)(d >> 32)), (uint32_t)q.seed,
                                          (uint32_t)(q.seed >> 32));
            if ((uint64_t)x.x * 1000u < rate) {  // (n < 2^30: the cuts leave the flag bits free)
                const uint32_t c1 = __umulhi(x.y, n + 1u), c2 = __umulhi(x.z, n + 1u);
                plan.x = (c1 < c2 ? c1 : c2) | FIM_FLAG;
                plan.y = (c1 < c2 ? c2 : c1) | ((uint64_t)x.w * 1000u < spm ? FIM_FLAG : 0u);
            }
        }
        q.plan[r] = plan;
        q.rec_len[r] = keep ? n + (plan.x & FIM_FLAG ? 4u : 1u) : 0u;
    }
}

// The element map of one document: segment index i (0 <= i <= e3) is <PRE> at s0, <SUF> at e1,
// <MID> at e2, eos at e3 and else source id t[i + d], d = d1 below e1, d2 below e2, d3 below e3
// (mod 2^32).  An untouched document has no sentinel position and d = 0.  This is the one text of
// the permutation: the gather's groups, its boundary loop and the carry kernel all go through it.
struct FimMap {
    uint32_t s0, e1, e2, e3, d1, d2, d3;
};
__device__ __forceinline__ FimMap fim_map(uint2 plan, uint32_t n) {
    FimMap m;
    if (!(plan.x & FIM_FLAG)) {
        m.s0 = m.e1 = m.e2 = ~0u;
        m.e3 = n;
        m.d1 = m.d2 = m.d3 = 0u;
        return m;
    }
    const uint32_t a = plan.x & ~FIM_FLAG, b = plan.y & ~FIM_FLAG;
    const bool spm = (plan.y & FIM_FLAG) != 0u;
    m.s0 = 0u;
    m.e1 = spm ? 1u : a + 1u;       // PSM: <PRE> t[0:a] <SUF>;  SPM: <PRE> <SUF>
    m.e2 = m.e1 + 1u + (n - b);     // ... t[b:n] <MID>
    m.e3 = n + 3u;                  // ... t[a:b] (PSM) / t[0:b] (SPM: prefix ++ middle is one run) eos
    m.d1 = ~0u;                     // i - 1
    m.d2 = b - (m.e1 + 1u);         // b + (i - e1 - 1)
    m.d3 = (spm ? 0u : a) - (m.e2 + 1u);
    return m;
}
// The id at segment index i of a kept record (n >= 1 ids from tok[base]): the load is issued for
// every i at a clamped address and the sentinel selected afterwards, so the loads of a group do
// not wait for one another.
__device__ __forceinline__ int32_t fim_id(const PackFimParams &q, const FimMap &m, uint32_t base, uint32_t n, uint32_t i) {
    const uint32_t j = i + (i < m.e1 ? m.d1 : i < m.e2 ? m.d2 : m.d3);
    const int32_t t = (int32_t)q.tok[base + (j < n ? j : n - 1u)];
    return i >= m.e3 ? q.eos : i == m.s0 ? q.pre : i == m.e1 ? q.suf : i == m.e2 ? q.mid : t;
}

struct FimElem {
    int32_t id, pos;
};
// Stream position p (c0 <= p < L) of record r: its id and position_id.
__device__ __forceinline__ FimElem fim_elem(const PackFimParams &q, uint32_t r, uint32_t p, uint32_t start) {
    const uint32_t n = q.rec_cnt[r];
    const uint32_t row0 = p / (uint32_t)q.S * (uint32_t)q.S;
    FimElem e;
    e.id = fim_id(q, fim_map(q.plan[r], n), q.rec_tok[r], n, p - start);
    e.pos = (int32_t)(p - (start > row0 ? start : row0));
    return e;
}

__device__ __forceinline__ void fim_store4(int32_t *__restrict__ o, uint32_t p, uint32_t end, const int32_t (&v)[4]) {
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
// positions inside one record loads that record's plan word, count and first id once, derives the
// map in registers and issues its four id loads independently -- also when the group crosses a
// sentinel or a run boundary of the permutation; only a group that crosses a record boundary, the
// carry or the stream's end takes the chained loop.
constexpr uint32_t FIM_WAVE_POS = 1024u;
constexpr uint32_t FIM_TILE = 4u * FIM_WAVE_POS;
__global__ __launch_bounds__(256) void k_pack_gather_fim(PackFimParams q) {
    const uint32_t S = (uint32_t)q.S, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / S, full = G * S;
    uint64_t gpad = ((uint64_t)G + (uint64_t)q.B - 1u) / (uint64_t)q.B * (uint64_t)q.B;
    if (gpad > (uint64_t)q.rows_cap) gpad = (uint64_t)q.rows_cap;
    const uint32_t end = (uint32_t)(gpad * S);  // (rows_cap * S < 2^32: checked by the host)
    const int lane = lane_id();
    for (uint64_t t0 = (uint64_t)blockIdx.x * FIM_TILE; t0 < end; t0 += (uint64_t)gridDim.x * FIM_TILE) {
        const uint32_t wb = (uint32_t)t0 + (uint32_t)(threadIdx.x >> 6) * FIM_WAVE_POS;  // the wave's first position
        if (wb >= end) continue;
        // wave-uniform: the record of the wave's first stream position past the carry (when it has one)
        uint32_t r = 0;
        const uint32_t wf = wb > c0 ? wb : c0;
        if (wf < full) r = pack_record_of(q.pk_off, 0u, R - 1u, wf);  // (full > c0: R > 0)
        for (uint32_t k = 0; k < FIM_WAVE_POS / 256u; ++k) {
            const uint32_t p0 = wb + 256u * k + 4u * (uint32_t)lane;
            if (p0 >= end) break;
            int32_t id[4], am[4], lab[4], pos[4];
            if (p0 >= full) {  // padding rows only
#pragma unroll
                for (int w = 0; w < 4; ++w) id[w] = 0, am[w] = 1, lab[w] = -100, pos[w] = 0;
            } else {
                uint32_t start = 0, next = 0;
                const uint32_t pf = p0 > c0 ? p0 : c0;  // the lane's first position past the carry
                if (pf < full) {  // (pf >= wf, and pk_off[r] <= the lane's last position: r is at or below pf's record)
                    r = pack_record_near(q.pk_off, r, R - 1u, pf);
                    start = q.pk_off[r];
                    next = q.pk_off[r + 1u];
                }
                if (p0 >= c0 && p0 + 3u < next && p0 + 3u < full) {
                    const uint32_t n = q.rec_cnt[r], base = q.rec_tok[r], i0 = p0 - start;
                    const FimMap m = fim_map(q.plan[r], n);
                    const uint32_t row0 = p0 / S * S;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const uint32_t p = p0 + (uint32_t)w;
                        const uint32_t rs = p - row0 < S ? row0 : p / S * S;  // (a row end inside the group)
                        id[w] = lab[w] = fim_id(q, m, base, n, i0 + (uint32_t)w);
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
                            id[w] = lab[w] = q.carry_ids[p];
                            pos[w] = q.carry_pos[p];
                            am[w] = 1;
                        } else {
                            while (p >= next) {  // p < L = pk_off[R]: ends at a record of length > 0
                                ++r;
                                start = next;
                                next = q.pk_off[r + 1u];
                            }
                            const FimElem e = fim_elem(q, r, p, start);
                            id[w] = lab[w] = e.id;
                            pos[w] = e.pos;
                            am[w] = 1;
                        }
                    }
                }
            }
            fim_store4(q.ids, p0, end, id);
            fim_store4(q.am, p0, end, am);
            fim_store4(q.lab, p0, end, lab);
            fim_store4(q.pos, p0, end, pos);
        }
    }
}

// stream[G S :) and its position_ids in the row it will open -> the other half of the carry, through
// the same element map; the new length, the call's row count and the handle's record counter (one
// workgroup; fewer than S <= 2048 elements).
__global__ __launch_bounds__(256) void k_pack_carry_fim(PackFimParams q) {
    const uint32_t S = (uint32_t)q.S, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / S, full = G * S, n = L - full;
    for (uint32_t x = threadIdx.x; x < n; x += 256u) {
        const uint32_t p = full + x;
        if (p < c0) {  // (G == 0: the old carry stays in front)
            q.new_ids[x] = q.carry_ids[p];
            q.new_pos[x] = q.carry_pos[p];
        } else {
            const uint32_t r = pack_record_of(q.pk_off, 0u, R - 1u, p);
            const FimElem e = fim_elem(q, r, p, q.pk_off[r]);
            q.new_ids[x] = e.id;
            q.new_pos[x] = e.pos;
        }
    }
    if (threadIdx.x == 0) {
        *q.new_len = n;
        *q.d_rows = G;
        *q.rec_seen += (uint64_t)q.R;  // (k_fim_plan, the only reader, ran before this launch on the stream)
    }
}

hipError_t launch_fim_plan(const PackFimParams &q, hipStream_t st) {
    const int64_t want = (q.R + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 1024 ? want : 1024);
    hipLaunchKernelGGL(k_fim_plan, dim3(grid), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t launch_pack_fim_rows(const PackFimParams &q, hipStream_t st) {
    const int64_t tiles = (q.rows_cap * q.S + (int64_t)FIM_TILE - 1) / (int64_t)FIM_TILE;
    const unsigned grid = (unsigned)(tiles < 1 ? 1 : tiles < 16384 ? tiles : 16384);
    hipLaunchKernelGGL(k_pack_gather_fim, dim3(grid), dim3(256), 0, st, q);
    hipLaunchKernelGGL(k_pack_carry_fim, dim3(1), dim3(256), 0, st, q);
    return hipGetLastError();
}

}  // namespace sdl
