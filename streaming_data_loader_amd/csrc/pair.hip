// pair.hip -- one [CLS] A [SEP] B [SEP] row per example of two texts (sdl_config.pair = 1, DESIGN.md
// §3 "Sentence pairs") on gfx950.
//
// The tokenizer ran over 2 * n_pairs text ranges of one arena (A_r = range 2r, B_r = range 2r + 1)
// and launch_records left each range's first id and id count, so a pair's row is a function of
// four words: rec_tok / rec_cnt of ranges 2r and 2r + 1.  The kept lengths (k_a, k_b) are
// tokenizers' longest_first truncation in closed form (pair_kept) and every column's source
// follows from comparing it with five boundaries -- no loop over ids, nothing divergent beyond
// the selects and the short chunk search below.  The ids are read from the WordPiece chunk lists
// themselves (list_index.hpp), not from a dense copy: a row keeps at most S - 3 of its pair's ids
// and the kept ones are the first of each side, so the copy moved every id of the call for the
// few a row reads (DESIGN.md §4 "Sentence pairs": 0.076 ms of a 0.131 ms stage).  The work item
// is a lane's four consecutive columns of one row, flat over (row, column group): at S = 8 a wave
// writes 32 rows, at S = 2048 an eighth of one, by the same code, and with S on the 4-int grid
// consecutive lanes store consecutive 16 bytes across row ends.  Every column of the three planes
// is written for every row up to the next multiple of B: nothing a previous call left in the
// buffers shows.
#include "device_util.hpp"
#include "kernels.hpp"
#include "rows_device.hpp"

namespace sdl {

struct PairKept {
    uint32_t a, b;
};
// tokenizers' TruncationStrategy::LongestFirst (right, stride 0) for n_a + n_b ids into M: the
// longer side is cut to what the shorter leaves, both to halves once the shorter exceeds its half;
// on a tie A counts as the shorter, so B gets the odd id.
__device__ __forceinline__ PairKept pair_kept(uint32_t na, uint32_t nb, uint32_t M) {
    // (64-bit sum: ids are bounded by the arena's bytes, < 2^32 each)
    if ((uint64_t)na + nb <= M) return PairKept{na, nb};
    uint32_t lo = na < nb ? na : nb, hi = na < nb ? nb : na;
    hi = lo > M ? lo : (lo > M - lo ? lo : M - lo);
    if ((uint64_t)lo + hi > M) {
        lo = M / 2u;
        hi = M / 2u + M % 2u;
    }
    return na <= nb ? PairKept{lo, hi} : PairKept{hi, lo};
}

__global__ __launch_bounds__(256) void k_rows_pair(PairParams q) {
    const uint32_t S = (uint32_t)q.S, Q = (S + 3u) >> 2;  // column groups a row
    const bool vec = (S & 3u) == 0u;                       // 16-byte aligned rows
    const uint32_t G = (uint32_t)q.n_pairs;
    const uint64_t total = (uint64_t)q.rows_end * Q;       // (rows_end * S < 2^32: checked by the host)
    if (blockIdx.x == 0 && threadIdx.x == 0) {             // the label kernels' one segment: a row per pair
        q.rb[0] = 0u;
        q.rb[1] = G;
        q.row_off[G] = G;
    }
    for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256u) {
        const uint32_t g = (uint32_t)t / Q, j0 = 4u * ((uint32_t)t - g * Q);
        int32_t id[4], am[4], tt[4];
        if (g >= G) {  // rows of the last batch nobody filled: the unpaired task's initial values
#pragma unroll
            for (int w = 0; w < 4; ++w) id[w] = 0, am[w] = 1, tt[w] = 0;
        } else {
            const uint32_t ta = q.rec_tok[2u * g], tb = q.rec_tok[2u * g + 1u];
            // the chunks each side's ids lie in (those of its own bytes); a lane's ids have rising
            // indices, so each search starts at the chunk of the one before
            ListBracket ba = list_bracket(q.off[2u * g], q.off[2u * g + 1u], q.n_lists);
            ListBracket bb = list_bracket(q.off[2u * g + 1u], q.off[2u * g + 2u], q.n_lists);
            const PairKept k = pair_kept(q.rec_cnt[2u * g], q.rec_cnt[2u * g + 1u], S - 3u);
            // columns: [CLS] at 0, a at [1, c1), [SEP] at c1, b at [c2, c3), [SEP] at c3, padding from c4
            const uint32_t c1 = 1u + k.a, c2 = c1 + 1u, c3 = c2 + k.b, c4 = c3 + 1u;
            if (j0 == 0u) {
                q.row_off[g] = g;
                q.row_rec[g] = g;
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t j = j0 + (uint32_t)w;
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
                id[w] = v;
                am[w] = j < c4 ? 1 : 0;
                tt[w] = j >= c2 && j < c4 ? 1 : 0;
            }
        }
        const size_t row = (size_t)g * S;
        store4(q.ids + row, (int)j0, (int)S, vec, id[0], id[1], id[2], id[3]);
        store4(q.am + row, (int)j0, (int)S, vec, am[0], am[1], am[2], am[3]);
        store4(q.tt + row, (int)j0, (int)S, vec, tt[0], tt[1], tt[2], tt[3]);
    }
}

hipError_t launch_rows_pair(const PairParams &q, hipStream_t st) {
    if (q.S < 3 || q.n_pairs < 0 || q.rows_end < q.n_pairs || q.rows_end * (int64_t)q.S >= ((int64_t)1 << 32))
        return hipErrorInvalidValue;
    const int64_t want = (q.rows_end * ((q.S + 3) / 4) + 255) / 256;
    const unsigned grid = (unsigned)(want < 1 ? 1 : want < 16384 ? want : 16384);
    hipLaunchKernelGGL(k_rows_pair, dim3(grid), dim3(256), 0, st, q);
    return hipGetLastError();
}

}  // namespace sdl
