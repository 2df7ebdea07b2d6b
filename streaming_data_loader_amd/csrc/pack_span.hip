// pack_span.hip -- T5 pre-training chunks cut from the concatenated document stream and corrupted
// on the device (sdl_config.pack = 1 under the span task with span_policy 1, DESIGN.md §3 "Packed
// span rows") on gfx950: t5.data.preprocessors.span_corruption / HF run_t5_mlm_flax.py.
//
// The call's stream is  carry ++ concat over kept records r of (ids_r ++ [</s>]),  pk_off[r] the
// stream position where record r starts (pack.hip's lengths kernel and the seeded scan), and row g
// of the call is the corruption of chunk stream[g N, (g + 1) N): N > S source ids chosen on the host
// so that the corrupted chunk -- u kept ids and m sentinels -- fills the S input columns.
// k_rows_span_t5 holds a row of at most S ids of one record; here a wave owns one chunk of N ids
// that may span many records:
//   1. the chunk's ids into LDS: one wave-uniform binary search in pk_off for the record of the
//      chunk's first position past the carry, every lane gallops on from there (pack_search.hpp) to
//      the records of its own positions (groups of four, two groups a round), ids from the dense
//      array, </s> at a record's end, the carry's from the carry buffer; a round's eight loads are
//      all issued before the first LDS write;
//   2. (t, m) from the host's counts table; the t - 1 noise keys and the u - 1 keep keys -- N - 2
//      words -- are drawn in ONE loop over the Philox blocks of both domains into one key array
//      (noise keys at key[0 .. t - 1), keep keys behind them), then span_select_cuts runs twice on
//      keys already in LDS and a ballot and prefix count per 64 keys compacts the cuts into span starts;
//   3. lanes turn the starts into plan entries, scatter each span's first input and label position
//      into marks (in the keys' place), and a max-scan over the marks writes both planes
//      position-parallel, 16 bytes a lane where the width is a multiple of 4.
// The row is chunk 0 of record q, the row's packed index on the handle: the keys, cuts and planes
// are those of the unpacked policy row with these ids (§3 "Span policies" Cuts and Row).
//
// LDS: 8 NP bytes a wave (NP = N rounded up to 4: ids, then keys / marks) beside 1.5 KB of plan and
// start tables a wave; four waves a block up to N = 1792, two up to PACK_SPAN_MAX_N = 3584.
#include "device_util.hpp"
#include "kernels.hpp"
#include "pack_search.hpp"
#include "rows_device.hpp"
#include "span_noise.hpp"

// Diagnostic builds only (build.py build_pack_span_ablations): 1 = the keys from a multiply in the
// place of Philox; 2 = no keys, no selection and no compaction, spans of even lengths.  Their rows
// are not the contract's: they say where k_pack_span_rows' time goes.
#ifndef SDL_PACK_SPAN_ABLATE
#define SDL_PACK_SPAN_ABLATE 0
#endif

namespace sdl {

constexpr int PACK_SPAN_TAB = 128;  // plan entries and span starts a row holds in LDS (m <= 100)

struct PackSpanWave {  // the wave, as span_noise.hpp asks for it
    __device__ __forceinline__ uint32_t lane() const { return (uint32_t)lane_id(); }
    __device__ __forceinline__ uint32_t lanes() const { return 64u; }
    __device__ __forceinline__ uint32_t sum(uint32_t x) const {
        return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_sum(x), 63);
    }
    __device__ __forceinline__ uint32_t min(uint32_t x) const {
        DPP_SCAN_ID(x, min_u32r, 0xFFFFFFFFu);
        return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
    }
};

// one lane's LDS writes before the others' reads (a wave: program order)
__device__ __forceinline__ void pack_span_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// A lane's place in the stream: the record of its last position, that record's extent, id count
// and first id.  Positions only rise.
struct PackSpanCursor {
    uint32_t r, start, next, n, base;
};

__device__ __forceinline__ void pack_span_seek(const PackSpanParams &q, PackSpanCursor &c, uint32_t r) {
    c.r = r;
    c.start = q.pk_off[r];
    c.next = q.pk_off[r + 1u];
    c.n = q.rec_cnt[r];
    c.base = q.rec_tok[r];
}

// Where stream position p (c0 <= p < L, at or past the cursor's record start) has its id, or null
// for a record's closing </s>.  far: the record may lie many records on (a lane's next group) --
// gallop; else step (runs of dropped records share an offset and are stepped over).
__device__ __forceinline__ const int32_t *pack_span_src(const PackSpanParams &q, PackSpanCursor &c, uint32_t p, bool far) {
    if (p >= c.next) {
        uint32_t r = far ? pack_record_near(q.pk_off, c.r, (uint32_t)q.R - 1u, p) : c.r;
        uint32_t next = q.pk_off[r + 1u];
        while (p >= next) {  // p < L = pk_off[R]: ends at a record of length > 0
            ++r;
            next = q.pk_off[r + 1u];
        }
        pack_span_seek(q, c, r);
    }
    const uint32_t i = p - c.start;
    return i >= c.n ? nullptr : reinterpret_cast<const int32_t *>(q.tok) + c.base + i;
}

// Positions [0, W) of one plane of a row, lane L holding 256 m + 4 L + w: the owner span of each
// position = the max-scan of `mk` (span s marked at its first position); val(q, owner) gives the
// value; positions >= end get tail(q).  One 16-byte store a lane when W is a multiple of 4.
template <class Val, class Tail>
__device__ __forceinline__ void pack_span_plane(int32_t *__restrict__ o, int W, int end, const uint16_t *mk, Val val,
                                                Tail tail) {
    const int lane = lane_id();
    uint32_t carry = 0;
    const bool vec = (W & 3) == 0;
    for (int b = 0; b < W; b += 256) {
        const int q0 = b + 4 * lane;
        uint32_t own[4], run = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int q = q0 + w;
            const uint32_t m = q < end ? (uint32_t)mk[q] : 0u;
            run = max_u32(run, m);
            own[w] = run;
        }
        uint32_t x = run;
        DPP_SCAN(x, max_u32);
        // (the DPP read once, unconditionally: under a partial exec mask it reads 0 from the inactive neighbours)
        const uint32_t prev = wave_prev(x), last = (uint32_t)lane_bcast((int)x, 63);
        const uint32_t before = max_u32(prev, carry);
        carry = max_u32(carry, last);
        int32_t v[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int q = q0 + w;
            v[w] = q < end ? val(q, max_u32(own[w], before)) : tail(q);
        }
        store4(o, q0, W, vec, v[0], v[1], v[2], v[3]);
    }
}

// The wave's slice of the block's LDS.
struct PackSpanLds {
    int32_t *rid;    // [NP] the chunk's ids
    uint32_t *key;   // [NP] the keys of both domains, then the marks: mk[S] u16 | mk2[LW] u16
    uint2 *tl;       // [PACK_SPAN_TAB] plan entries
    uint16_t *nb;    // [PACK_SPAN_TAB] where each span's noise ids start
    uint16_t *ka;    // [PACK_SPAN_TAB] ... and its kept ids
    const int32_t *extra;  // [100] the sentinels (the block's)
};

// A row nobody filled: T5Data::new's values.
__device__ __forceinline__ void pack_span_pad_row(const PackSpanParams &q, uint32_t g, int lane) {
    const int S = q.S, LW = q.LW;
    int32_t *ids_o = q.ids + (size_t)g * S, *am_o = q.am + (size_t)g * S, *lb_o = q.lab + (size_t)g * LW;
    for (int j0 = 4 * lane; j0 < S; j0 += 256) {
        store4(ids_o, j0, S, (S & 3) == 0, 0, 0, 0, 0);
        store4(am_o, j0, S, (S & 3) == 0, 1, 1, 1, 1);
    }
    for (int j0 = 4 * lane; j0 < LW; j0 += 256) store4(lb_o, j0, LW, (LW & 3) == 0, -100, -100, -100, -100);
}

// Output row g = the corruption of stream[row0, row0 + n) (n = N; the flush row: row0 = 0 and
// n = c0, all of it the carry) as chunk 0 of record `rec`.
__device__ __forceinline__ void pack_span_row(const PackSpanParams &q, uint32_t g, uint32_t row0, int n, uint32_t c0,
                                              uint64_t rec, const PackSpanLds &lds, int lane) {
    const int S = q.S, LW = q.LW;
    int32_t *ids_o = q.ids + (size_t)g * S, *am_o = q.am + (size_t)g * S, *lb_o = q.lab + (size_t)g * LW;
    int32_t *rid = lds.rid;
    uint32_t *key = lds.key;
    uint16_t *mk = reinterpret_cast<uint16_t *>(key), *mk2 = mk + S;
    uint2 *tl = lds.tl;
    uint16_t *nb = lds.nb, *ka = lds.ka;
    const PackSpanWave wv{};
    auto extra = [&](uint32_t s) -> int32_t { return lds.extra[s < 100u ? s : 99u]; };

    const uint32_t tm = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.counts[n]);
    const int t = (int)(tm & 0xFFFFu), m = (int)(tm >> 16), u = n - t;
    // (none of these once sdl_batcher_create took the config: u + m, t + m and m never decrease with n)
    if (m + 1 > SPAN_MAX_SENTINELS || t + m + 1 > LW || u + m > S) {
        pack_span_pad_row(q, g, lane);
        return;
    }

    // 1. the chunk's ids
    PackSpanCursor cur{};
    const uint32_t wf = row0 > c0 ? row0 : c0;
    if (wf < row0 + (uint32_t)n)  // (then R > 0 and wf < L)
        pack_span_seek(q, cur, (uint32_t)__builtin_amdgcn_readfirstlane(
                                   (int)pack_record_of(q.pk_off, 0u, (uint32_t)q.R - 1u, wf)));
    for (int j0 = 0; j0 < n; j0 += 512) {
        const int32_t *src[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = j0 + 256 * (e >> 2) + 4 * lane + (e & 3);
            src[e] = nullptr;
            if (j < n) {
                const uint32_t p = row0 + (uint32_t)j;
                src[e] = p < c0 ? q.carry_ids + p : pack_span_src(q, cur, p, (e & 3) == 0);  // (the carry lies in row 0)
            }
        }
        int32_t v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = src[e] ? *src[e] : q.eos;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = j0 + 256 * (e >> 2) + 4 * lane + (e & 3);
            if (j < n) rid[j] = v[e];
        }
    }

    // 2. the cuts of both compositions
    if (lane == 0) {
        nb[0] = 0;
        ka[0] = 0;
    }
    if (SDL_PACK_SPAN_ABLATE >= 2) {
        for (int s = lane; s < m; s += 64) {
            nb[s] = (uint16_t)((int64_t)s * t / m);
            ka[s] = (uint16_t)((int64_t)s * u / m);
        }
        pack_span_fence();
    } else if (m > 1) {  // (then t >= 2 and u >= 2)
        const uint32_t nkN = (uint32_t)t - 1u, nkK = (uint32_t)u - 1u;  // cut candidates i = 1..nk, key[i - 1]
        const uint32_t nbN = nkN / 4u + 1u, nbK = nkK / 4u + 1u;        // Philox blocks q with 4 q <= nk
        for (uint32_t b = (uint32_t)lane; b < nbN + nbK; b += 64u) {
            const bool keep = b >= nbN;
            const uint32_t qb = keep ? b - nbN : b, nk = keep ? nkK : nkN, at = keep ? nkN : 0u;
            const uint32_t D = keep ? SPAN_KEEP_DOMAIN : SPAN_NOISE_DOMAIN;
#if SDL_PACK_SPAN_ABLATE >= 1
            const uint32_t h = (4u * qb + D + (uint32_t)rec) * 0x9E3779B1u;
            const uint4 c = make_uint4(h, h + 0x9E3779B1u, h + 2u * 0x9E3779B1u, h + 3u * 0x9E3779B1u);
#else
            const uint4 c = philox4x32_10(make_uint4(qb, D, (uint32_t)rec, (uint32_t)(rec >> 32)), (uint32_t)q.seed,
                                          (uint32_t)(q.seed >> 32));
#endif
            const uint32_t w[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) {
                const uint32_t i = 4u * qb + e;
                if (i >= 1u && i <= nk) key[at + i - 1u] = w[e];
            }
        }
        pack_span_fence();
#pragma unroll 1
        for (int dom = 0; dom < 2; ++dom) {
            const uint32_t *kd = dom ? key + nkN : key;
            const uint32_t nk = dom ? nkK : nkN;
            uint16_t *st = dom ? ka : nb;
            const SpanSel ss = span_select_cuts(kd, nk, (uint32_t)m - 1u, wv);
            uint32_t rank = 1;  // span 0 starts at 0
            for (uint32_t b0 = 0; b0 < nk; b0 += 64u) {
                const uint32_t j = b0 + (uint32_t)lane;
                const bool f = j < nk && span_selected(ss, kd[j], j);
                const uint64_t bal = __ballot(f);
                const uint32_t at = rank + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
                if (f && at < (uint32_t)PACK_SPAN_TAB) st[at] = (uint16_t)(j + 1u);
                rank += (uint32_t)__popcll(bal);
            }
        }
        pack_span_fence();  // (the marks overwrite the keys)
    }

    // 3. the plan, the marks and the planes
    const int np = m > 0 ? m : 1;
    for (int s = lane; s < np; s += 64) {
        if (m == 0) {
            tl[0] = make_uint2(0u | 1u << 16, 0u);  // the row's one id, kept; no span
        } else {
            const uint32_t A = ka[s], a = (s + 1 < m ? (uint32_t)ka[s + 1] : (uint32_t)u) - A;
            const uint32_t Bn = nb[s], b = (s + 1 < m ? (uint32_t)nb[s + 1] : (uint32_t)t) - Bn;
            const SpanEntry e = span_plan_entry((uint32_t)s, A, a, Bn, b);
            tl[s] = make_uint2(e.x, e.y);
        }
    }
    for (int j = 2 * lane; j < S + LW; j += 128) *reinterpret_cast<uint32_t *>(mk + j) = 0u;
    pack_span_fence();
    for (int p = lane; p < np; p += 64) {
        const uint2 e = tl[p];
        const int lp = (int)(e.x & 0xFFFFu), ip = (int)(e.y & 0xFFFFu);
        const int ap = ip - lp + 2 * p;
        if (lp < S) mk[lp] = (uint16_t)p;
        if (m > 0 && ap < LW) mk2[ap] = (uint16_t)p;
    }
    pack_span_fence();
    const int L = u + m;
    pack_span_plane(
        ids_o, S, L, mk,
        [&](int x, uint32_t o) -> int32_t {
            const uint2 e = tl[o];
            const int off = x - (int)(e.x & 0xFFFFu), ge = (int)(e.x >> 16);
            return off < ge ? rid[(int)(e.y & 0xFFFFu) + off] : extra(o);
        },
        [&](int) -> int32_t { return 0; });
    for (int j0 = 4 * lane; j0 < S; j0 += 256)
        store4(am_o, j0, S, (S & 3) == 0, j0 < L ? 1 : 0, j0 + 1 < L ? 1 : 0, j0 + 2 < L ? 1 : 0, j0 + 3 < L ? 1 : 0);
    const int ap_end = t + m;
    const int32_t fin = extra((uint32_t)m);  // the closing sentinel
    pack_span_plane(
        lb_o, LW, ap_end, mk2,
        [&](int x, uint32_t o) -> int32_t {
            const uint2 e = tl[o];
            const int lp = (int)(e.x & 0xFFFFu), ge = (int)(e.x >> 16), ip = (int)(e.y & 0xFFFFu);
            const int off = x - (ip - lp + 2 * (int)o);
            return off == 0 ? extra(o) : rid[ip + ge + off - 1];
        },
        [&](int x) -> int32_t { return x == ap_end ? fin : -100; });
    pack_span_fence();  // (the wave's next row rewrites the ids, the plan and the marks)
}

// The block's LDS cut into its waves' slices; the sentinels once a block.
__device__ __forceinline__ PackSpanLds pack_span_lds(const PackSpanParams &q, int32_t *s_extra, uint2 *s_tab,
                                                     uint16_t *s_start, int32_t *s_dyn, int wid) {
    const int NP = (q.N + 3) & ~3;
    if (threadIdx.x < 100) s_extra[threadIdx.x] = q.extra_ids[threadIdx.x];
    __syncthreads();
    PackSpanLds l;
    l.rid = s_dyn + (size_t)wid * 2 * NP;
    l.key = reinterpret_cast<uint32_t *>(l.rid + NP);
    l.tl = s_tab + wid * PACK_SPAN_TAB;
    l.nb = s_start + wid * 2 * PACK_SPAN_TAB;
    l.ka = l.nb + PACK_SPAN_TAB;
    l.extra = s_extra;
    return l;
}

// The three planes of the call's rows: rows [0, G) the stream's chunks, [G, end) the padding rows
// up to the next multiple of B.  The grid is sized from the upper bound rows_cap -- the row count
// stays on the device -- and the packed index of row g is the handle's counter (the half the last
// call wrote; k_pack_span_carry writes the other one) plus g.
__global__ __launch_bounds__(256) void k_pack_span_rows(PackSpanParams q) {
    __shared__ int32_t s_extra[100];
    __shared__ uint2 s_tab[4 * PACK_SPAN_TAB];
    __shared__ uint16_t s_start[4 * 2 * PACK_SPAN_TAB];
    extern __shared__ int32_t s_dyn[];
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nw = blockDim.x >> 6;
    const PackSpanLds lds = pack_span_lds(q, s_extra, s_tab, s_start, s_dyn, wid);
    const uint32_t N = (uint32_t)q.N, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / N;
    uint64_t gpad = ((uint64_t)G + (uint64_t)q.B - 1u) / (uint64_t)q.B * (uint64_t)q.B;
    if (gpad > (uint64_t)q.rows_cap) gpad = (uint64_t)q.rows_cap;
    const uint32_t end = (uint32_t)gpad;  // (rows_cap * N < 2^32: checked by the host)
    const uint64_t q0 = *q.row_cnt;
    for (uint32_t g = blockIdx.x * nw + (uint32_t)wid; g < end; g += gridDim.x * nw) {
        if (g < G) pack_span_row(q, g, g * N, (int)N, c0, q0 + g, lds, lane);
        else pack_span_pad_row(q, g, lane);
    }
}

// stream[G N :) -> the other half of the carry, the new length, the row counter advanced by G and
// the call's row count (one workgroup; fewer than N <= 3584 ids).
__global__ __launch_bounds__(256) void k_pack_span_carry(PackSpanParams q) {
    const uint32_t N = (uint32_t)q.N, R = (uint32_t)q.R;
    const uint32_t c0 = q.pk_off[0], L = q.pk_off[R];
    const uint32_t G = L / N, full = G * N, n = L - full;
    for (uint32_t x = threadIdx.x; x < n; x += 256u) {
        const uint32_t p = full + x;
        if (p < c0) {  // (G == 0: the old carry stays in front)
            q.new_ids[x] = q.carry_ids[p];
        } else {
            PackSpanCursor cur;
            pack_span_seek(q, cur, pack_record_of(q.pk_off, 0u, R - 1u, p));
            const int32_t *src = pack_span_src(q, cur, p, false);
            q.new_ids[x] = src ? *src : q.eos;
        }
    }
    if (threadIdx.x == 0) {
        *q.new_len = n;
        *q.new_row_cnt = *q.row_cnt + G;
        *q.d_rows = G;
    }
}

// The flush row: the carry's c ids corrupted with n = c and the next packed index into row 0; rows
// 1 .. B - 1 (and row 0 when c == 0) get the padding rows' values; the other half's length becomes
// 0 and its counter the old one plus the row.
__global__ __launch_bounds__(256) void k_pack_span_flush(PackSpanParams q) {
    __shared__ int32_t s_extra[100];
    __shared__ uint2 s_tab[4 * PACK_SPAN_TAB];
    __shared__ uint16_t s_start[4 * 2 * PACK_SPAN_TAB];
    extern __shared__ int32_t s_dyn[];
    const int lane = lane_id();
    const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t nw = blockDim.x >> 6;
    const PackSpanLds lds = pack_span_lds(q, s_extra, s_tab, s_start, s_dyn, wid);
    uint32_t c = *q.carry_len;
    if (c >= (uint32_t)q.N) c = 0u;  // (never: a carry is shorter than a chunk)
    const uint64_t q0 = *q.row_cnt;
    const uint32_t end = (uint32_t)((int64_t)q.B < q.rows_cap ? (int64_t)q.B : q.rows_cap);
    for (uint32_t g = blockIdx.x * nw + (uint32_t)wid; g < end; g += gridDim.x * nw) {
        if (g == 0u && c > 0u) pack_span_row(q, 0u, 0u, (int)c, c, q0, lds, lane);
        else pack_span_pad_row(q, g, lane);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *q.new_len = 0u;
        *q.new_row_cnt = q0 + (c > 0u ? 1u : 0u);
        *q.d_rows = c > 0u ? 1u : 0u;
    }
}

static bool pack_span_ok(const PackSpanParams &q) {
    return q.S >= 4 && q.S <= 2048 && q.LW == q.S / 4 && q.N >= q.S && q.N <= PACK_SPAN_MAX_N && q.B > 0 && q.R >= 0 &&
           q.R < ((int64_t)1 << 32) - 1 && q.rows_cap >= 0 && q.rows_cap * (int64_t)q.N < ((int64_t)1 << 32) &&
           q.counts && q.extra_ids && q.ids && q.am && q.lab;
}
// waves a block and their LDS: ids and keys, 8 NP bytes a wave
static int pack_span_waves(const PackSpanParams &q, size_t *dyn) {
    const int NP = (q.N + 3) & ~3;
    const int waves = 32 * NP <= 56 * 1024 ? 4 : 2;
    *dyn = (size_t)waves * 2 * NP * sizeof(int32_t);
    return waves;
}

hipError_t launch_pack_span_rows(const PackSpanParams &q, hipStream_t st) {
    if (!pack_span_ok(q)) return hipErrorInvalidValue;
    size_t dyn;
    const int waves = pack_span_waves(q, &dyn);
    const int64_t want = (q.rows_cap + waves - 1) / waves;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 16384 ? want : 16384);
    hipLaunchKernelGGL(k_pack_span_rows, dim3(grid), dim3(64 * waves), dyn, st, q);
    hipLaunchKernelGGL(k_pack_span_carry, dim3(1), dim3(256), 0, st, q);
    return hipGetLastError();
}

hipError_t launch_pack_span_flush(const PackSpanParams &q, hipStream_t st) {
    if (!pack_span_ok(q)) return hipErrorInvalidValue;
    size_t dyn;
    const int waves = pack_span_waves(q, &dyn);
    const int64_t want = ((int64_t)q.B + waves - 1) / waves;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 4096 ? want : 4096);
    hipLaunchKernelGGL(k_pack_span_flush, dim3(grid), dim3(64 * waves), dyn, st, q);
    return hipGetLastError();
}

}  // namespace sdl
