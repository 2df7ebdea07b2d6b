// zstd.hip -- Zstandard frames decoded on the device (sdl_zstd_inflate_device).
//
// Block sizes stand in the block headers, so every block start is known without decoding.  The
// entropy decode (Huffman literals, FSE sequences) therefore runs for all blocks of all frames at
// once; what a block cannot know alone -- the repeat-offset history entering it, its position in
// the output -- is carried symbolically and closed by two thin per-frame chains:
//
//   1 k_zs_index     lane per frame    frame header, block headers -> block records
//   2 k_zs_parse     lane per block    literals / sequences section headers
//   3 k_zs_link      lane per frame    who defines each block's tree and tables; arena bases
//   4 k_zs_decode    2 waves per block tables in LDS; wave 0: literals -> literal arena (the four
//                                      Huffman streams in four lanes); wave 1: sequences -> records
//                                      with symbolic repeat offsets, the block's history map and size
//   5 k_zs_chain     lane per frame    maps composed into incoming histories, output bases, sizes
//   6 k_zs_literals  workgroup/block   literal runs, raw and RLE blocks to their final place
//   7 k_zs_matches   workgroup/frame   blocks in order, in windows of 8 KiB of output: markers
//                                      substituted, offsets checked, every match byte's source found
//                                      by pointer jumping in LDS, then all match bytes copied at once
//   8 k_zs_xxh       4 lanes per frame XXH64, low 32 bits against the frame's checksum
//
// No workgroup waits for another: stages are ordered by launch order, stage 7 by __syncthreads().
// Every loop over input-derived counts is bounded (and leaves with ZS_E_STALL where the bound is a
// guard).  All format knowledge, the bit reader included, is zstd_format.hpp, which the host model
// (tests/zstd_host_model.cpp) runs under sanitizers; the kernels add the parallel copies.
#include "device_util.hpp"
#include "kernels.hpp"

namespace sdl {
namespace {

using namespace zs;

constexpr int ZS_LANES = 128;   // stages 1, 2, 3, 5: threads per workgroup (one frame / block each)
constexpr int ZS_WRITE = 256;   // stage 6

__global__ __launch_bounds__(ZS_LANES) void k_zs_index(const uint8_t *__restrict__ zst, uint64_t len,
                                                       const uint64_t *__restrict__ foff, uint64_t n, Frame *frames,
                                                       Block *blocks, const uint32_t *__restrict__ first_block,
                                                       uint32_t *__restrict__ nblk, uint32_t block_cap) {
    const uint64_t f = (uint64_t)blockIdx.x * ZS_LANES + threadIdx.x;
    if (f >= n) return;
    Frame F;
    F.first_block = blocks ? first_block[f] : 0;
    const uint64_t a = foff[f], z = foff[f + 1];
    if (z < a || z > len) {
        F.src = F.end = 0;
        F.n_blocks = 0;
        F.skippable = F.has_fcs = F.checksum = F.block_max = 0;
        F.fcs = 0;
        F.sum_off = F.out_base = F.out_size = F.lit_total = F.seq_total = 0;
        F.status = E_RANGE;
    } else {
        index_frame(zst, a, z, (uint32_t)f, F, blocks, block_cap);
    }
    if (blocks)
        frames[f] = F;
    else
        nblk[f] = F.n_blocks;
}

__global__ __launch_bounds__(ZS_LANES) void k_zs_parse(const uint8_t *__restrict__ zst, const Frame *__restrict__ frames,
                                                       Block *blocks, uint32_t nb) {
    const uint32_t b = blockIdx.x * ZS_LANES + threadIdx.x;
    if (b >= nb) return;
    Block &B = blocks[b];
    if (B.type != 2 || B.status) return;
    Sections s;
    B.status = parse_sections(zst + B.src, B.size, frames[B.frame].block_max, s);
    B.sec = s;
}

// totals (64-bit, so the host can refuse a call before a 32-bit scan of these could wrap):
// [0] literal bytes, [1] sequence records, [2] output bytes
__global__ __launch_bounds__(ZS_LANES) void k_zs_link(Frame *frames, Block *blocks, uint64_t n,
                                                      uint32_t *__restrict__ lit_tot, uint32_t *__restrict__ seq_tot,
                                                      unsigned long long *totals) {
    const uint64_t f = (uint64_t)blockIdx.x * ZS_LANES + threadIdx.x;
    if (f >= n) return;
    link_frame(frames[f], blocks);
    const uint32_t lt = frames[f].status ? 0 : frames[f].lit_total, sq = frames[f].status ? 0 : frames[f].seq_total;
    lit_tot[f] = lt;
    seq_tot[f] = sq;
    if (lt) atomicAdd(&totals[0], (unsigned long long)lt);
    if (sq) atomicAdd(&totals[1], (unsigned long long)sq);
}

// Two waves a block: wave 0 builds the Huffman table and decodes the literals (the four streams in
// four lanes), wave 1 builds the three sequence tables and decodes the sequences -- the two need
// nothing of each other (the sequences only the literals' count, from the header).
__global__ __launch_bounds__(128) void k_zs_decode(const uint8_t *__restrict__ zst, const Frame *__restrict__ frames,
                                                   Block *blocks, uint32_t nb, const uint32_t *__restrict__ lit_base,
                                                   const uint32_t *__restrict__ seq_base, uint8_t *__restrict__ lit_arena,
                                                   SeqRec *__restrict__ seq_arena) {
    __shared__ Tables T;
    __shared__ int32_t lit_status, seq_status;
    const uint32_t b = blockIdx.x;
    if (b >= nb) return;
    Block &B = blocks[b];
    const uint32_t f = B.frame;
    if (frames[f].status || B.type != 2 || B.status) return;  // (uniform)
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (threadIdx.x == 0) {
        block_setup_literals(zst, blocks, B, T);
        lit_status = T.status;
    }
    if (threadIdx.x == 64) {
        block_setup_sequences(zst, blocks, B, T);
        seq_status = T.seq_status;
    }
    __syncthreads();
    if (wave == 0 && !lit_status) {
        // the block's extent of the literal arena: [lit, lit + regen) -- the bases are the scans of
        // exactly these sizes (k_zs_link), so the extent lies inside the arena
        uint8_t *lit = lit_arena + lit_base[f] + B.lit_base;
        const uint32_t regen = B.sec.regen;
        if (B.sec.lit_type == 0) {
            const uint8_t *src = zst + B.src + B.sec.streams;  // parse_sections: streams + regen <= the block
            for (uint32_t i = lane; i < regen; i += 64) lit[i] = src[i];
        } else if (B.sec.lit_type == 1) {
            const uint8_t v = zst[B.src + B.sec.streams];
            for (uint32_t i = lane; i < regen; i += 64) lit[i] = v;
        } else if (lane < 4) {
            const int32_t st = block_lit_stream(zst, B, T, (uint32_t)lane, lit);
            if (st) atomicMax(&lit_status, st);
        }
    } else if (wave == 1 && lane == 0 && !seq_status) {
        // ... and of the sequence arena: [rec, rec + nseq)
        seq_status = block_sequences(zst, B, T, frames[f].block_max, seq_arena + seq_base[f] + B.seq_base, nullptr);
    }
    __syncthreads();
    if (threadIdx.x == 0) B.status = lit_status ? lit_status : seq_status;
}

__global__ __launch_bounds__(ZS_LANES) void k_zs_chain(Frame *frames, Block *blocks, uint64_t n,
                                                       uint32_t *__restrict__ out_size, unsigned long long *totals) {
    const uint64_t f = (uint64_t)blockIdx.x * ZS_LANES + threadIdx.x;
    if (f >= n) return;
    chain_frame(frames[f], blocks);
    out_size[f] = frames[f].out_size;
    if (frames[f].out_size) atomicAdd(&totals[2], (unsigned long long)frames[f].out_size);
}

// n bytes src -> dst by the 64 lanes of a wave
__device__ __forceinline__ void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n, int lane) {
    for (uint32_t i = lane; i < n; i += 64) dst[i] = src[i];
}

__global__ __launch_bounds__(ZS_WRITE) void k_zs_literals(const uint8_t *__restrict__ zst, const Frame *__restrict__ frames,
                                                          const Block *__restrict__ blocks, uint32_t nb,
                                                          const uint32_t *__restrict__ lit_base,
                                                          const uint32_t *__restrict__ seq_base,
                                                          const uint8_t *__restrict__ lit_arena,
                                                          const SeqRec *__restrict__ seq_arena,
                                                          const uint32_t *__restrict__ ooff, uint8_t *__restrict__ out) {
    const uint32_t b = blockIdx.x;
    if (b >= nb) return;
    const Block &B = blocks[b];
    const Frame &F = frames[B.frame];
    if (F.status) return;
    // the block's extent of the output: [dst, dst + size), inside the frame's [0, F.out_size)
    const uint32_t size = B.out_size;
    if ((uint64_t)B.out_base + size > F.out_size) return;
    uint8_t *dst = out + ooff[B.frame] + B.out_base;
    const int tid = (int)threadIdx.x, lane = tid & 63;
    if (B.type == 0) {
        const uint8_t *src = zst + B.src;  // block_header: size bytes of content
        for (uint32_t i = tid; i < size; i += ZS_WRITE) dst[i] = src[i];
        return;
    }
    if (B.type == 1) {
        const uint8_t v = zst[B.src];
        for (uint32_t i = tid; i < size; i += ZS_WRITE) dst[i] = v;
        return;
    }
    const uint8_t *lit = lit_arena + lit_base[B.frame] + B.lit_base;
    const SeqRec *rec = seq_arena + seq_base[B.frame] + B.seq_base;
    const uint32_t nseq = B.sec.nseq, regen = B.sec.regen;
    for (uint32_t base = 0; base < nseq; base += ZS_WRITE) {  // (uniform trip count: the ballots below)
        const uint32_t i = base + tid;
        uint32_t ll = 0, from = 0, to = 0;
        if (i < nseq) {
            const SeqRec r = rec[i];
            from = i ? rec[i - 1].lit_end : 0;
            // decode_sequences: lit_end rises to <= regen, dst >= its literals, dst + ml <= size
            if (r.lit_end >= from && r.lit_end <= regen && r.dst <= size && r.lit_end - from <= r.dst) {
                ll = r.lit_end - from;
                to = r.dst - ll;
            }
        }
        if (ll <= 32)
            for (uint32_t j = 0; j < ll; ++j) dst[to + j] = lit[from + j];
        uint64_t longs = __ballot(ll > 32);
        while (longs) {
            const int l = __ffsll((unsigned long long)longs) - 1;
            longs &= longs - 1;
            wave_copy(dst + __shfl(to, l), lit + __shfl(from, l), __shfl(ll, l), lane);
        }
    }
    uint32_t from = 0, to = 0;
    if (nseq) {
        from = rec[nseq - 1].lit_end;
        to = rec[nseq - 1].dst + (rec[nseq - 1].ml_kind & ML_MASK);
    }
    if (from <= regen && (uint64_t)to + (regen - from) <= size)
        for (uint32_t i = tid; i < regen - from; i += ZS_WRITE) dst[to + i] = lit[from + i];
}

// Stage 7.  A match copies bytes that earlier matches may have produced, so sequences cannot all
// copy at once; but which byte every output byte comes FROM is known without copying anything.
// One workgroup takes a frame, block by block, in windows of ZS_WIN output bytes:
//   a. every sequence overlapping the window writes, for its match bytes p, the source p - offset
//      into ptr[] (LDS); literal bytes (already in place, stage 6) stay marked SELF;
//   b. pointer jumping, ptr[j] = ptr[ptr[j]], until every entry names a literal byte of the window
//      or a byte before the window (both final): <= log2(ZS_WIN) + 1 rounds, whatever the chains;
//   c. every match byte loads its root and is stored.
// Offsets are checked against the bytes the frame has produced (E_FAR).  Rounds and windows are
// ordered by __syncthreads(); nothing waits for another workgroup.
constexpr int ZS_MATCH = 1024;
constexpr uint32_t ZS_WIN = 8192;
constexpr uint32_t ZS_SELF = 0xFFFFFFFFu;

__global__ __launch_bounds__(ZS_MATCH) void k_zs_matches(Frame *frames, const Block *__restrict__ blocks,
                                                         const uint32_t *__restrict__ seq_base,
                                                         const SeqRec *__restrict__ seq_arena,
                                                         const uint32_t *__restrict__ ooff, uint8_t *out) {
    __shared__ uint32_t ptr[ZS_WIN];  // per window byte: the frame position it copies from, or ZS_SELF
    __shared__ uint32_t s_next;
    __shared__ int32_t s_status;
    const uint32_t f = blockIdx.x;
    Frame &F = frames[f];
    if (F.status || F.skippable) return;
    const uint32_t tid = threadIdx.x;
    uint8_t *fo = out + ooff[f];
    const uint32_t fsize = F.out_size;
    if (tid == 0) s_status = OK;
    __syncthreads();
    for (uint32_t bi = 0; bi < F.n_blocks; ++bi) {
        const Block &B = blocks[F.first_block + bi];
        if (B.type != 2 || B.sec.nseq == 0) continue;
        const SeqRec *rec = seq_arena + seq_base[f] + B.seq_base;
        const uint32_t nseq = B.sec.nseq, bbase = B.out_base, bsize = B.out_size;
        if ((uint64_t)bbase + bsize > fsize) break;  // (chain_frame: the blocks tile the frame's extent)
        const uint32_t in[3] = {B.rep_in[0], B.rep_in[1], B.rep_in[2]};
        uint32_t cursor = 0;  // the first sequence that may reach into the window (uniform)
        for (uint32_t w0 = 0; w0 < bsize; w0 += ZS_WIN) {  // block-relative window [w0, w1)
            const uint32_t w1 = w0 + ZS_WIN < bsize ? w0 + ZS_WIN : bsize, wlen = w1 - w0;
            const uint32_t fw0 = bbase + w0;  // the window's first byte in the frame
            for (uint32_t j = tid; j < wlen; j += ZS_MATCH) ptr[j] = ZS_SELF;
            if (tid == 0) s_next = nseq;
            __syncthreads();
            // a. sequences from the cursor on, while they start inside the window (<= nseq / ZS_MATCH + 1 trips)
            for (uint32_t base = cursor;; base += ZS_MATCH) {
                const uint32_t i = base + tid;
                bool more = false;
                if (i < nseq) {
                    const SeqRec r = rec[i];
                    const uint32_t ml = r.ml_kind & ML_MASK, d = r.dst;
                    if (d < w1) {
                        more = tid == ZS_MATCH - 1;  // the whole batch started inside: look at the next one
                        if (d + ml > w0) {
                            const uint32_t o = rep_resolve(RepSlot{r.ml_kind >> 30, r.off}, in);
                            // the offset against the bytes the frame has produced; the match inside its block
                            if (o == 0 || o > bbase + d || d + ml > bsize) {
                                s_status = E_FAR;
                            } else {
                                const uint32_t p0 = d > w0 ? d : w0, p1 = d + ml < w1 ? d + ml : w1;
                                for (uint32_t p = p0; p < p1; ++p) ptr[p - w0] = bbase + p - o;
                            }
                        }
                    }
                    if (d + ml > w1 || d >= w1) atomicMin(&s_next, i);  // it reaches past the window: the next cursor
                }
                if (!__syncthreads_or(more)) break;
            }
            if (s_status) break;  // (uniform: written before the barrier above)
            cursor = s_next;
            // b. pointer jumping; a source is always before its byte, so there are no cycles, and a
            // racing read sees an older or a newer ancestor, either of which is one
            int round = 0;
            for (; round < 16; ++round) {
                bool changed = false;
                for (uint32_t j = tid; j < wlen; j += ZS_MATCH) {
                    const uint32_t src = ptr[j];
                    if (src != ZS_SELF && src >= fw0) {
                        const uint32_t up = ptr[src - fw0];
                        if (up != ZS_SELF) {
                            ptr[j] = up;
                            changed = true;
                        }
                    }
                }
                if (!__syncthreads_or(changed)) break;
            }
            if (round == 16) {  // (2^13 bytes need 13 halvings: unreachable)
                if (tid == 0) s_status = E_STALL;
                __syncthreads();
                break;
            }
            // c. the roots are literal bytes of the window or bytes before it: final, and no byte
            // written here is one
            for (uint32_t j = tid; j < wlen; j += ZS_MATCH) {
                const uint32_t src = ptr[j];
                if (src != ZS_SELF) fo[fw0 + j] = fo[src];
            }
            __syncthreads();  // the window's bytes are written before the next window reads them
        }
        if (s_status) break;
    }
    __syncthreads();
    if (tid == 0 && s_status) F.status = s_status;
}

__global__ __launch_bounds__(64) void k_zs_xxh(const uint8_t *__restrict__ zst, Frame *frames,
                                               const uint32_t *__restrict__ ooff, const uint8_t *__restrict__ out) {
    __shared__ uint64_t acc[4];
    const uint32_t f = blockIdx.x;
    Frame &F = frames[f];
    if (F.status || F.skippable || !F.checksum) return;
    const uint8_t *p = out + ooff[f];
    const uint64_t len = F.out_size, stripes = len / 32;
    const int lane = (int)threadIdx.x;
    if (lane < 4) {
        uint64_t v = xxh_lane_seed((uint32_t)lane);
        const uint8_t *q = p + lane * 8;
        uint64_t s = 0;
        for (; s + 8 <= stripes; s += 8, q += 256) {  // the loads of eight stripes ahead of their rounds
            uint64_t x[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) memcpy(&x[k], q + 32 * k, 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) v = xxh_round(v, x[k]);
        }
        for (; s < stripes; ++s, q += 32) v = xxh_round(v, le64(q));
        acc[lane] = v;
    }
    __syncthreads();
    if (lane == 0) {
        const uint64_t v[4] = {acc[0], acc[1], acc[2], acc[3]};
        const uint64_t h = xxh_finish(v, p + stripes * 32, len);
        if ((uint32_t)h != le32(zst + F.sum_off)) F.status = E_CHECKSUM;  // index_frame: sum_off + 4 <= the frame's end
    }
}

__global__ __launch_bounds__(ZS_LANES) void k_zs_status(const Frame *__restrict__ frames, uint64_t n,
                                                        int32_t *__restrict__ status, uint32_t *bad) {
    const uint64_t f = (uint64_t)blockIdx.x * ZS_LANES + threadIdx.x;
    if (f >= n) return;
    const int32_t s = frames[f].status;
    status[f] = s;
    if (s) {
        atomicAdd(&bad[0], 1u);
        atomicMin(&bad[1], (uint32_t)f);
    }
}

unsigned grid_for(uint64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

hipError_t launch_zs_index(const uint8_t *zst, uint64_t len, const uint64_t *foff, uint64_t n, zs::Frame *frames,
                           zs::Block *blocks, const uint32_t *first_block, uint32_t *nblk, uint32_t block_cap,
                           hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_zs_index, dim3(grid_for(n, ZS_LANES)), dim3(ZS_LANES), 0, st, zst, len, foff, n, frames, blocks,
                       first_block, nblk, block_cap);
    return hipGetLastError();
}

hipError_t launch_zs_parse(const uint8_t *zst, const zs::Frame *frames, zs::Block *blocks, uint32_t nb, hipStream_t st) {
    if (!nb) return hipSuccess;
    hipLaunchKernelGGL(k_zs_parse, dim3(grid_for(nb, ZS_LANES)), dim3(ZS_LANES), 0, st, zst, frames, blocks, nb);
    return hipGetLastError();
}

hipError_t launch_zs_link(zs::Frame *frames, zs::Block *blocks, uint64_t n, uint32_t *lit_tot, uint32_t *seq_tot,
                          unsigned long long *totals, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_zs_link, dim3(grid_for(n, ZS_LANES)), dim3(ZS_LANES), 0, st, frames, blocks, n, lit_tot, seq_tot,
                       totals);
    return hipGetLastError();
}

hipError_t launch_zs_decode(const uint8_t *zst, const zs::Frame *frames, zs::Block *blocks, uint32_t nb,
                            const uint32_t *lit_base, const uint32_t *seq_base, uint8_t *lit, zs::SeqRec *seq,
                            hipStream_t st) {
    if (!nb) return hipSuccess;
    hipLaunchKernelGGL(k_zs_decode, dim3(nb), dim3(128), 0, st, zst, frames, blocks, nb, lit_base, seq_base, lit, seq);
    return hipGetLastError();
}

hipError_t launch_zs_chain(zs::Frame *frames, zs::Block *blocks, uint64_t n, uint32_t *out_size,
                           unsigned long long *totals, hipStream_t st) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_zs_chain, dim3(grid_for(n, ZS_LANES)), dim3(ZS_LANES), 0, st, frames, blocks, n, out_size, totals);
    return hipGetLastError();
}

hipError_t launch_zs_write(const uint8_t *zst, zs::Frame *frames, const zs::Block *blocks, uint32_t nb, uint64_t n,
                           const uint32_t *lit_base, const uint32_t *seq_base, const uint8_t *lit, const zs::SeqRec *seq,
                           const uint32_t *ooff, uint8_t *out, bool check, int32_t *status, uint32_t *bad,
                           hipStream_t st, hipEvent_t *ev) {
    if (!n) return hipSuccess;
    if (nb)
        hipLaunchKernelGGL(k_zs_literals, dim3(nb), dim3(ZS_WRITE), 0, st, zst, frames, blocks, nb, lit_base, seq_base, lit,
                           seq, ooff, out);
    if (ev && hipEventRecord(ev[0], st) != hipSuccess) return hipGetLastError();
    hipLaunchKernelGGL(k_zs_matches, dim3((unsigned)n), dim3(ZS_MATCH), 0, st, frames, blocks, seq_base, seq, ooff, out);
    if (ev && hipEventRecord(ev[1], st) != hipSuccess) return hipGetLastError();
    if (check) hipLaunchKernelGGL(k_zs_xxh, dim3((unsigned)n), dim3(64), 0, st, zst, frames, ooff, out);
    hipLaunchKernelGGL(k_zs_status, dim3(grid_for(n, ZS_LANES)), dim3(ZS_LANES), 0, st, frames, n, status, bad);
    return hipGetLastError();
}

}  // namespace sdl
