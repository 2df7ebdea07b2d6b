// pack.hip -- CLM rows packed from the concatenated document stream (sdl_config.pack = 1,
// DESIGN.md §3 "Packed rows") on gfx950.
//
// The unpacked rows kernels go record -> rows (rec_rows -> row_off -> row_rec, a wave per row of
// one record).  A packed row holds many records and a record spans many rows, so the map is
// inverted here: the call's stream is  carry ++ concat over kept records r of (ids_r ++ [eos]),
// pk_off[r] is the stream position where record r starts (an exclusive scan of the packed
// lengths seeded with the carry length), and the planes are [rows, S] row-major -- output
// element p IS stream position p.  So the gather runs over the flat index p, each wave finds the
// record of its first position by one binary search in pk_off, and every plane is written in
// whole 16-byte groups that are aligned for every S, also off the 4-int grid.
//
// A document's end is a record's end (pk_off), never an id compared with eos: a record's text may
// hold the literal <|endoftext|>.  The carry keeps its position_ids beside its ids for the same
// reason.
#include "device_util.hpp"
#include "kernels.hpp"

namespace sdl {

// Per record: its packed length (the ids and one trailing eos, or 0 when dropped) into rec_len
// (sdl_device_rows.d_record_rows); thread 0 seeds the scan with the carry length.
__global__ __launch_bounds__(256) void k_pack_lengths(PackParams q) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) q.pk_off[0] = *q.carry_len;
    for (int64_t r = i; r < q.R; r += (int64_t)gridDim.x * 256) {
        const uint32_t n = q.rec_cnt[r];
        q.rec_len[r] = n >= 1u && n + 1u >= (uint32_t)(q.min_ids > 0 ? q.min_ids : 0) ? n + 1u : 0u;
    }
}

// The record holding stream position p, c0 <= p < L: the last r in [lo, hi] with pk_off[r] <= p
// (records of length 0 share their successor's offset and are never the answer).  The caller
// guarantees pk_off[lo] <= p.
__device__ __forceinline__ uint32_t pack_record_of(const uint32_t *__restrict__ pk_off, uint32_t lo, uint32_t hi,
                                                   uint32_t p) {
    while (lo < hi) {
        const uint32_t m = lo + (hi - lo + 1u) / 2u;
        if (pk_off[m] <= p) lo = m;
        else hi = m - 1u;
    }
    return lo;
}

struct PackElem {
    int32_t id, pos;
};
// Stream position p (c0 <= p < L) of record r: its id and position_id.
__device__ __forceinline__ PackElem pack_elem(const PackParams &q, uint32_t r, uint32_t p, uint32_t start) {
    const uint32_t i = p - start, n = q.rec_cnt[r];
    const uint32_t row0 = p / (uint32_t)q.S * (uint32_t)q.S;
    PackElem e;
    e.id = i >= n ? q.eos : (int32_t)q.tok[q.rec_tok[r] + i];
    e.pos = (int32_t)(p - (start > row0 ? start : row0));
    return e;
}

__device__ __forceinline__ void pack_store4(int32_t *__restrict__ o, uint32_t p, uint32_t end, const int32_t (&v)[4]) {
    if (p + 4u <= end) {  // the planes stream out: non-temporal, this pass does not read them again
        typedef int32_t v4i __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(v4i{v[0], v[1], v[2], v[3]}, reinterpret_cast<v4i *>(o + p));
    } else {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (p + (uint32_t)w < end) o[p + w] = v[w];
    }
}

// The same for a caller whose answer lies near lo (a lane after its wave's search, or after its
// own last position): a galloping search, one or two loads where a binary search over every
// record takes log2 R dependent ones.
__device__ __forceinline__ uint32_t pack_record_near(const uint32_t *__restrict__ pk_off, uint32_t lo, uint32_t last,
                                                     uint32_t p) {
    uint32_t step = 1u;
    while (lo + step <= last && pk_off[lo + step] <= p) {
        lo += step;
        step <<= 1;
    }
    const uint32_t hi = lo + step - 1u < last ? lo + step - 1u : last;
    return pack_record_of(pk_off, lo, hi, p);
}

// The four planes over the flat output index.  A wave takes PACK_WAVE_POS consecutive positions
// in rounds of 64 4-position groups (256 positions, one 16-byte store a lane and plane); a
// workgroup's four waves take a tile of 4 x PACK_WAVE_POS, and the tiles are strided over a grid
// sized from the upper bound rows_cap * S -- the row count stays on the device.  The wave finds
// the record of its first position by one wave-uniform binary search in pk_off (log2 R dependent
// loads: the reason a wave takes more than one round), each lane then its own record from there,
// and from its own last record in the rounds after.  Positions [0, G S) are the stream,
// [G S, end) the padding rows up to the next multiple of B with their initial values.
constexpr uint32_t PACK_WAVE_POS = 1024u;
constexpr uint32_t PACK_TILE = 4u * PACK_WAVE_POS;
__global__ __launch_bounds__(256) void k_pack_gather(PackParams q) {
    const uint32_t S = (uint32_t)q.S, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / S, full = G * S;
    uint64_t gpad = ((uint64_t)G + (uint64_t)q.B - 1u) / (uint64_t)q.B * (uint64_t)q.B;
    if (gpad > (uint64_t)q.rows_cap) gpad = (uint64_t)q.rows_cap;
    const uint32_t end = (uint32_t)(gpad * S);  // (rows_cap * S < 2^32: checked by the host)
    const int lane = lane_id();
    for (uint64_t t0 = (uint64_t)blockIdx.x * PACK_TILE; t0 < end; t0 += (uint64_t)gridDim.x * PACK_TILE) {
        const uint32_t wb = (uint32_t)t0 + (uint32_t)(threadIdx.x >> 6) * PACK_WAVE_POS;  // the wave's first position
        if (wb >= end) continue;
        // wave-uniform: the record of the wave's first stream position past the carry (when it has one)
        uint32_t r = 0;
        const uint32_t wf = wb > c0 ? wb : c0;
        if (wf < full) r = pack_record_of(q.pk_off, 0u, R - 1u, wf);  // (full > c0: R > 0)
        for (uint32_t k = 0; k < PACK_WAVE_POS / 256u; ++k) {
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
                    // the usual group, inside one record: its count and first id once, then four
                    // independent id loads (the general loop below chains them one after another)
                    const uint32_t n = q.rec_cnt[r], base = q.rec_tok[r], i0 = p0 - start;
                    const uint32_t row0 = p0 / S * S;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const uint32_t p = p0 + (uint32_t)w, i = i0 + (uint32_t)w;
                        const uint32_t rs = p - row0 < S ? row0 : p / S * S;  // (a row end inside the group)
                        id[w] = lab[w] = i >= n ? q.eos : (int32_t)q.tok[base + i];
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
                            const PackElem e = pack_elem(q, r, p, start);
                            id[w] = lab[w] = e.id;
                            pos[w] = e.pos;
                            am[w] = 1;
                        }
                    }
                }
            }
            pack_store4(q.ids, p0, end, id);
            pack_store4(q.am, p0, end, am);
            pack_store4(q.lab, p0, end, lab);
            pack_store4(q.pos, p0, end, pos);
        }
    }
}

// stream[G S :) and its position_ids in the row it will open -> the other half of the carry, the
// new length and the call's row count (one workgroup; fewer than S <= 2048 elements).
__global__ __launch_bounds__(256) void k_pack_carry(PackParams q) {
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
            const PackElem e = pack_elem(q, r, p, q.pk_off[r]);
            q.new_ids[x] = e.id;
            q.new_pos[x] = e.pos;
        }
    }
    if (threadIdx.x == 0) {
        *q.new_len = n;
        *q.d_rows = G;
    }
}

// The flush row: the carry's c ids in row 0, the plain orientation (columns >= c: input_ids 0,
// attention_mask 0, labels -100, position_ids 0); rows 1 .. B - 1 get the padding rows' initial
// values; the other half's length becomes 0.  c == 0 emits no row.
__global__ __launch_bounds__(256) void k_pack_flush(PackParams q) {
    const uint32_t S = (uint32_t)q.S, c = *q.carry_len;
    uint64_t rows = (uint64_t)q.B;
    if (rows > (uint64_t)q.rows_cap) rows = (uint64_t)q.rows_cap;
    const uint64_t end = rows * S;
    for (uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x; p < end; p += (uint64_t)gridDim.x * 256u) {
        int32_t id = 0, am = 1, lab = -100, pos = 0;
        if (p < S && c > 0u) {
            am = 0;
            if (p < c) {
                id = lab = q.carry_ids[p];
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

hipError_t launch_pack_lengths(const PackParams &q, hipStream_t st) {
    const int64_t want = (q.R + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 1024 ? want : 1024);
    hipLaunchKernelGGL(k_pack_lengths, dim3(grid), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t launch_pack_rows(const PackParams &q, hipStream_t st) {
    const int64_t tiles = (q.rows_cap * q.S + (int64_t)PACK_TILE - 1) / (int64_t)PACK_TILE;
    const unsigned grid = (unsigned)(tiles < 1 ? 1 : tiles < 16384 ? tiles : 16384);
    hipLaunchKernelGGL(k_pack_gather, dim3(grid), dim3(256), 0, st, q);
    hipLaunchKernelGGL(k_pack_carry, dim3(1), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t launch_pack_flush(const PackParams &q, hipStream_t st) {
    const int64_t want = ((int64_t)q.B * q.S + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 4096 ? want : 4096);
    hipLaunchKernelGGL(k_pack_flush, dim3(grid), dim3(256), 0, st, q);
    return hipGetLastError();
}

}  // namespace sdl
