// pack_bestfit.hip -- packed CLM rows by best-fit-decreasing (sdl_batcher_set_best_fit on a pack = 1
// handle, DESIGN.md §3 "Best-fit rows") on gfx950.
//
// pack.hip cuts the concatenated stream every S ids, so almost every row starts inside a document.
// Here a record's segment (its n ids and the eos, L = n + 1) gives floor(L / S) full pieces of S ids,
// one row each, and -- when L mod S > 0 -- one tail that stays whole.  The tails of a window of W
// records are placed by best-fit-decreasing: longest first, each into the open row with the least
// room that still takes it (the row that came to have that room last, among equals), else into a
// new row.  Rows are lists of pieces with padding behind them, so nothing of the gather applies:
//
//   k_bestfit_plan   one wave a window.  Lengths and the full-piece prefix with DPP scans; the
//                    tails sorted in LDS by a bitonic network over composite keys
//                    (S - length) << 12 | index in the window (unique, so no stable sort is needed);
//                    then the serial placement.  The rooms of the open rows are a bitmap in
//                    registers: lane j holds the 64-bit word of rooms [64 j, 64 j + 63] (S <= 4096),
//                    "least room >= l" is a mask, a ballot, two read-lanes and two counts of
//                    trailing zeros.  The rows of one room are a stack, head[room] and a next link
//                    per row; the link shares a 32-bit word with the row's piece count, so a
//                    placement is three dependent LDS round trips (key, head, row word).  Afterwards
//                    the wave scans the piece counts and scatters the pieces so that a row's pieces
//                    are one contiguous run in placement order, 16 bytes each.
//   scan             launch_exclusive_scan over the windows' row counts: window k's first row.
//   k_bestfit_rows   a wave a row, four rows a workgroup.  A full row copies S ids of one record.
//                    A tail row stages its run of pieces in LDS (up to 64; a longer run is read
//                    where it lies), each lane finds the piece of its 4-column group by a binary
//                    search on the columns and loads four independent ids when the group lies
//                    inside one piece.  Groups are aligned on the flat plane index, so the 16-byte
//                    non-temporal stores are aligned for every S; a group that straddles two rows
//                    is written element by element from both sides.
//
// LDS of k_bestfit_plan (dynamic): 14 P + 2 S bytes -- keys, results and row words 4 P each, ranks
// 2 P, heads 2 S.  At W = 4096 and S = 4096 that is 64 KiB, two waves a CU of gfx950's 160 KiB; at
// W = 1024 and S = 512, 15 KiB and ten.  The kernel is bound by the placement's dependent LDS
// latency, not by occupancy: a wave is one window.
#include "device_util.hpp"
#include "kernels.hpp"
#include "pack_search.hpp"

namespace sdl {

constexpr uint32_t BF_NIL = 0xFFFFu;     // no next row in a room's stack
constexpr uint32_t BF_NO_TAIL = ~0u;     // the key of a record without a tail: sorts behind every tail

__global__ __launch_bounds__(64) void k_bestfit_plan(BestFitParams q) {
    extern __shared__ uint32_t bf_lds[];
    const uint32_t S = (uint32_t)q.S, W = (uint32_t)q.W, P = (uint32_t)q.P, R = (uint32_t)q.R;
    uint32_t *keys = bf_lds;                 // [P] sorted: (S - length) << 12 | index in the window
    uint32_t *res = keys + P;                // [P] tail i (sorted order): row among the opened rows | column << 12
    uint32_t *rowst = res + P;               // [P] opened row: next row of its room's stack | pieces << 16
    uint16_t *rank = reinterpret_cast<uint16_t *>(rowst + P);  // [P] tail i: its place among its row's pieces
    uint16_t *head = rank + P;               // [S] room: the row that came to have it last
    const uint32_t lane = (uint32_t)lane_id();
    const uint32_t r0 = blockIdx.x * W;
    const uint32_t Wn = r0 >= R ? 0u : (R - r0 < W ? R - r0 : W);
    const uint32_t min_ids = (uint32_t)(q.min_ids > 0 ? q.min_ids : 0);

    // lengths: d_record_rows, the full pieces before each record, the tails' keys
    uint32_t nfull = 0, T = 0;
    for (uint32_t b = 0; b < P; b += 64u) {
        const uint32_t i = b + lane;
        uint32_t key = BF_NO_TAIL, f = 0;
        if (i < Wn) {
            const uint32_t n = q.rec_cnt[r0 + i];
            const uint32_t L = n >= 1u && n + 1u >= min_ids ? n + 1u : 0u;
            q.rec_len[r0 + i] = L;
            f = L / S;
            const uint32_t tl = L - f * S;
            if (tl) key = (S - tl) << 12 | i;
        }
        keys[i] = key;
        const uint32_t incl = wave_incl_sum(f);
        if (i < Wn) q.foff[r0 + i] = nfull + incl - f;
        nfull += lane_bcast(incl, 63);
        T += (uint32_t)__popcll(__ballot(key != BF_NO_TAIL));
    }

    // sort: ascending keys = decreasing length, equal lengths by ascending record index
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            __syncthreads();
            for (uint32_t t = lane; t < P / 2u; t += 64u) {
                const uint32_t lo = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), hi = lo | j;
                const uint32_t a = keys[lo], b = keys[hi];
                if ((a > b) == ((lo & k) == 0u)) {
                    keys[lo] = b;
                    keys[hi] = a;
                }
            }
        }
    }
    __syncthreads();

    // placement: wave-uniform, every lane runs it (the lanes differ in their word of the bitmap only)
    uint64_t bm = 0;  // bit b: room 64 lane + b has an open row
    uint32_t nopen = 0;
    for (uint32_t i = 0; i < T; ++i) {
        const uint32_t len = S - (keys[i] >> 12);
        const int cut = (int)len - (int)(64u * lane);  // this lane's rooms below len
        const uint64_t fit = cut <= 0 ? bm : cut >= 64 ? 0ull : bm & (~0ull << cut);
        const uint64_t any = __ballot(fit != 0ull);
        uint32_t row, col, pieces, left;
        if (any == 0ull) {  // no open row takes it: a new row behind the window's rows so far
            row = nopen++;
            col = 0u;
            pieces = 0u;
            left = S - len;
        } else {
            const int j = __builtin_ctzll(any);
            const uint32_t wl = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)fit, j);
            const uint32_t wh = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(fit >> 32), j);
            const uint32_t c = 64u * (uint32_t)j + (wl ? (uint32_t)__builtin_ctz(wl) : 32u + (uint32_t)__builtin_ctz(wh));
            row = head[c];  // pop the room's stack
            const uint32_t st = rowst[row], nx = st & 0xFFFFu;
            pieces = st >> 16;
            head[c] = (uint16_t)nx;
            if (nx == BF_NIL && lane == (uint32_t)j) bm &= ~(1ull << (c & 63u));
            col = S - c;
            left = c - len;
        }
        uint32_t nx = BF_NIL;
        if (left > 0u) {  // push on the stack of the room it has now (room 0 takes no tail: no stack)
            const bool mine = lane == left >> 6;
            if (__ballot(mine && (bm >> (left & 63u) & 1ull)) != 0ull) nx = head[left];
            head[left] = (uint16_t)row;
            if (mine) bm |= 1ull << (left & 63u);
        }
        rowst[row] = nx | (pieces + 1u) << 16;
        res[i] = row | col << 12;
        rank[i] = (uint16_t)pieces;
    }
    __syncthreads();

    // output: a row's pieces become one contiguous run (first piece | pieces << 16), in placement order
    uint32_t first = 0;
    for (uint32_t b = 0; b < nopen; b += 64u) {
        const uint32_t row = b + lane;
        const uint32_t c = row < nopen ? rowst[row] >> 16 : 0u;
        const uint32_t incl = wave_incl_sum(c);
        if (row < nopen) {
            const uint32_t v = (first + incl - c) | c << 16;
            rowst[row] = v;
            q.run[r0 + row] = v;
        }
        first += lane_bcast(incl, 63);
    }
    __syncthreads();
    for (uint32_t i = lane; i < T; i += 64u) {
        const uint32_t key = keys[i], len = S - (key >> 12), r = r0 + (key & 4095u);
        const uint32_t row = res[i] & 4095u, col = res[i] >> 12;
        const uint32_t d = (rowst[row] & 0xFFFFu) + rank[i];
        // the tail is the segment's last len entries: len - 1 ids and the eos
        if (d < Wn) q.piece[r0 + d] = make_uint4(col, len, q.rec_tok[r] + (q.rec_cnt[r] + 1u - len), r);
    }
    if (lane == 0u) {
        q.win_rows[blockIdx.x] = nfull + nopen;
        q.win_full[blockIdx.x] = nfull;
    }
}

__device__ __forceinline__ void bestfit_store4(int32_t *__restrict__ o, uint32_t p, uint32_t lo, uint32_t hi,
                                               const int32_t (&v)[4]) {
    if (p >= lo && p + 4u <= hi) {  // the planes stream out: non-temporal, this pass does not read them again
        typedef int32_t v4i __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(v4i{v[0], v[1], v[2], v[3]}, reinterpret_cast<v4i *>(o + p));
    } else {  // (a group shared with the row before or behind: each row writes its own elements)
#pragma unroll
        for (int w = 0; w < 4; ++w)
            if (p + (uint32_t)w >= lo && p + (uint32_t)w < hi) o[p + w] = v[w];
    }
}

// Rows [0, G) are the windows' rows, [G, the next multiple of B) the padding rows with their initial
// values.  A workgroup takes four consecutive rows a round, a wave one of them; the round count is
// the workgroup's, so the barrier around the staged piece table is reached by all four waves.
__global__ __launch_bounds__(256) void k_bestfit_rows(BestFitParams q) {
    __shared__ uint4 tab_lds[4][64];
    const uint32_t S = (uint32_t)q.S, W = (uint32_t)q.W, R = (uint32_t)q.R, nW = (uint32_t)q.nW;
    const uint32_t total = q.win_off[nW];
    const uint64_t G = total < (uint64_t)q.rows_cap ? total : (uint64_t)q.rows_cap;  // (total <= rows_cap: sdl_batcher::rows_capacity)
    uint64_t gpad = (G + (uint64_t)q.B - 1u) / (uint64_t)q.B * (uint64_t)q.B;
    if (gpad > (uint64_t)q.rows_cap) gpad = (uint64_t)q.rows_cap;
    const uint32_t lane = (uint32_t)lane_id(), wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) *q.d_rows = total;
    for (uint64_t g0 = (uint64_t)blockIdx.x * 4u; g0 < gpad; g0 += (uint64_t)gridDim.x * 4u) {
        const uint64_t g = g0 + wave;
        // 0: a padding row (or none); 1: a full piece of one record; 2: a run of tails
        int kind = 0;
        uint32_t base = 0, nrem = 0, cnt = 0;
        const uint4 *tab = nullptr;
        if (g < G) {
            const uint32_t k = pack_record_of(q.win_off, 0u, nW - 1u, (uint32_t)g);  // (windows without rows are never the answer)
            const uint32_t j = (uint32_t)g - q.win_off[k], nf = q.win_full[k], r0 = k * W;
            if (j < nf) {  // full piece j of the window: piece c of the last record with foff <= j
                const uint32_t r = pack_record_of(q.foff, r0, (R - r0 < W ? R : r0 + W) - 1u, j);
                const uint32_t c = j - q.foff[r];
                kind = 1;
                base = q.rec_tok[r] + c * S;
                nrem = q.rec_cnt[r] - c * S;  // ids of the record from this piece on: column nrem (if < S) is the eos
            } else {
                const uint32_t run = q.run[r0 + (j - nf)];
                kind = 2;
                cnt = run >> 16;
                tab = q.piece + r0 + (run & 0xFFFFu);
                if (cnt <= 64u) {
                    if (lane < cnt) tab_lds[wave][lane] = tab[lane];
                    tab = tab_lds[wave];
                }
            }
        }
        __syncthreads();
        if (g < gpad) {
            const uint32_t lo = (uint32_t)g * S, hi = lo + S;  // (rows_cap * S < 2^32: checked by the host)
            for (uint32_t p0 = (lo & ~3u) + 4u * lane; p0 < hi; p0 += 256u) {
                int32_t id[4], am[4], lab[4], pos[4];
                if (kind == 0) {
#pragma unroll
                    for (int w = 0; w < 4; ++w) id[w] = 0, am[w] = 1, lab[w] = -100, pos[w] = 0;
                } else if (kind == 1) {
#pragma unroll
                    for (int w = 0; w < 4; ++w) {  // (columns outside the row are not stored: clamped loads)
                        const uint32_t p = p0 + (uint32_t)w;
                        const uint32_t x = p < lo ? 0u : p >= hi ? S - 1u : p - lo;
                        id[w] = lab[w] = x < nrem ? (int32_t)q.tok[base + x] : q.eos;
                        am[w] = 1;
                        pos[w] = (int32_t)x;
                    }
                } else {
                    const uint32_t x0 = p0 < lo ? 0u : p0 - lo;
                    uint32_t a = 0, b = cnt - 1u;  // the last piece whose column is <= x0 (piece 0 lies at column 0)
                    while (a < b) {
                        const uint32_t m = a + (b - a + 1u) / 2u;
                        if (tab[m].x <= x0) a = m;
                        else b = m - 1u;
                    }
                    uint4 e = tab[a];
                    if (p0 >= lo && p0 + 3u < hi && x0 + 3u + 1u < e.x + e.y) {
                        // the usual group, inside one piece and before its eos: four independent id loads
                        const uint32_t o = x0 - e.x;
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            id[w] = lab[w] = (int32_t)q.tok[e.z + o + (uint32_t)w];
                            am[w] = 1;
                            pos[w] = (int32_t)(o + (uint32_t)w);
                        }
                    } else {
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            const uint32_t p = p0 + (uint32_t)w;
                            const uint32_t x = p < lo ? 0u : p >= hi ? S - 1u : p - lo;
                            while (x >= e.x + e.y && a + 1u < cnt) e = tab[++a];  // (pieces lie back to back)
                            const uint32_t o = x - e.x;
                            if (o < e.y) {
                                id[w] = lab[w] = o + 1u == e.y ? q.eos : (int32_t)q.tok[e.z + o];
                                am[w] = 1;
                                pos[w] = (int32_t)o;
                            } else {  // behind the last piece: the flush row's values
                                id[w] = 0, am[w] = 0, lab[w] = -100, pos[w] = 0;
                            }
                        }
                    }
                }
                bestfit_store4(q.ids, p0, lo, hi, id);
                bestfit_store4(q.am, p0, lo, hi, am);
                bestfit_store4(q.lab, p0, lo, hi, lab);
                bestfit_store4(q.pos, p0, lo, hi, pos);
            }
        }
        __syncthreads();  // (the next round stages over the table)
    }
}

hipError_t launch_bestfit_plan(const BestFitParams &q, hipStream_t st) {
    const size_t lds = (size_t)q.P * 14u + (((size_t)q.S + 1u) & ~(size_t)1u) * 2u;
    hipLaunchKernelGGL(k_bestfit_plan, dim3((unsigned)q.nW), dim3(64), lds, st, q);
    return hipGetLastError();
}

hipError_t launch_bestfit_rows(const BestFitParams &q, hipStream_t st) {
    const int64_t want = (q.rows_cap + 3) / 4;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 16384 ? want : 16384);
    hipLaunchKernelGGL(k_bestfit_rows, dim3(grid), dim3(256), 0, st, q);
    return hipGetLastError();
}

}  // namespace sdl
