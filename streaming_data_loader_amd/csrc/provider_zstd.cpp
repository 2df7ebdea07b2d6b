// provider_zstd.cpp -- the Provider's zstd step on the device (zstd.hip).  Its buffers are the
// handle's ZstdWork, its output the InflatedOut it shares with provider_gzip.cpp; it borrows the
// handle's stream and scan_tmp, and records its stages in the handle's profiling events.
#include "handle.hpp"

namespace {
// sdl_zstd_inflate_device (its host syncs fall into the stage before them)
const char *kZstdStageNames[] = {"zs_index", "zs_parse_link", "zs_decode", "zs_chain", "zs_literals", "zs_matches", "zs_checksum"};
const char *zs_reason(int32_t s) {
    static const char *const names[] = {"ok",
                                        "frame range outside the buffer, or not exactly one frame",
                                        "input ends inside the frame",
                                        "not a zstd frame (magic or a reserved header bit)",
                                        "the frame names a dictionary (Dictionary_ID)",
                                        "window log or offset code beyond the supported limit",
                                        "block type 3",
                                        "block size over Block_Maximum_Size",
                                        "bad literals section header",
                                        "bad Huffman tree description",
                                        "bad FSE table description",
                                        "bad sequences section header",
                                        "a bitstream did not end exactly",
                                        "offset before the frame's start",
                                        "decoded size differs from Frame_Content_Size",
                                        "XXH64 content checksum mismatch",
                                        "the decoder made no progress"};
    return s >= 0 && s < (int32_t)(sizeof(names) / sizeof(names[0])) ? names[s] : "unknown";
}
}  // namespace

extern "C" {
int sdl_zstd_inflate_device(sdl_batcher *h, const uint8_t *d_zst, uint64_t zst_len, const uint64_t *d_frame_offsets,
                            uint64_t n_frames, uint32_t flags, void *stream, sdl_inflated *out) {
    if (!h || !out || (n_frames && (!d_zst || !d_frame_offsets))) return fail(SDL_ERR_ARG, "null argument");
    if (flags & ~SDL_ZSTD_NO_CHECKSUM) return fail(SDL_ERR_ARG, "unknown flag bits");
    if (zst_len >= (1ull << 32)) return fail(SDL_ERR_CAPACITY, "zstd buffer must be < 4 GiB per call");
    if (n_frames >= (1ull << 31)) return fail(SDL_ERR_CAPACITY, "too many zstd frames in one call");
    if (((uintptr_t)d_zst & 15u) != 0) return fail(SDL_ERR_ARG, "d_zst must be 16-byte aligned");
    return guarded(SDL_ERR_ARG, SDL_ERR_ARG, [&]() -> int {
        hipStream_t st = stream ? (hipStream_t)stream : h->stream;
        const size_t n = (size_t)n_frames;
        h->inf.size.ensure(n + 1);
        h->inf.off.ensure(n + 1);
        h->inf.status.ensure(n + 1);
        h->inf.bad.ensure(2);
        h->zs.frames.ensure(n + 1);
        h->zs.nblk.ensure(n + 1);
        h->zs.first.ensure(n + 1);
        h->zs.lit_tot.ensure(n + 1);
        h->zs.seq_tot.ensure(n + 1);
        h->zs.lit_base.ensure(n + 1);
        h->zs.seq_base.ensure(n + 1);
        h->zs.totals.ensure(4);
        h->scan_tmp.ensure((size_t)scan_tmp_words(std::max<int64_t>((int64_t)n, 1)) + 1);
        unsigned long long totals[3] = {0, 0, 0};
        uint32_t nb = 0;
        h->n_stages = kStages;
        h->stage_names = kZstdStageNames;
        auto mark = [&](int i) {
            if (h->profiling) HIP_TRY(hipEventRecord(h->ev[i], st));
        };
        mark(0);
        if (n) {
            HIP_TRY(hipMemsetAsync(h->zs.totals.p, 0, 4 * sizeof(unsigned long long), st));
            // stage 1: count the blocks, scan, (sync: the block records are sized), fill
            HIP_TRY(launch_zs_index(d_zst, zst_len, d_frame_offsets, n_frames, h->zs.frames.p, nullptr, nullptr,
                                    h->zs.nblk.p, 0, st));
            HIP_TRY(launch_exclusive_scan(h->zs.nblk.p, h->zs.first.p, (int64_t)n, h->scan_tmp.p, st));
            HIP_TRY(hipMemcpyAsync(&nb, h->zs.first.p + n, sizeof(nb), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            // (a block is >= 3 bytes of a < 4 GiB input: the count cannot wrap)
            h->zs.blocks.ensure((size_t)nb + 1);
            HIP_TRY(launch_zs_index(d_zst, zst_len, d_frame_offsets, n_frames, h->zs.frames.p, h->zs.blocks.p,
                                    h->zs.first.p, h->zs.nblk.p, nb, st));
            mark(1);
            // stages 2, 3; (sync: the literal arena and the sequence records are sized)
            HIP_TRY(launch_zs_parse(d_zst, h->zs.frames.p, h->zs.blocks.p, nb, st));
            HIP_TRY(launch_zs_link(h->zs.frames.p, h->zs.blocks.p, n_frames, h->zs.lit_tot.p, h->zs.seq_tot.p,
                                   h->zs.totals.p, st));
            HIP_TRY(hipMemcpyAsync(totals, h->zs.totals.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            // the headers' sizes are untrusted until decoded: they bound the arenas, never a kernel's writes
            if (totals[0] >= (1ull << 32) - 64 || totals[1] >= (1ull << 28))
                return fail(SDL_ERR_CAPACITY, "zstd frames hold >= 4 GiB of literals or sequence records in one call");
            HIP_TRY(launch_exclusive_scan(h->zs.lit_tot.p, h->zs.lit_base.p, (int64_t)n, h->scan_tmp.p, st));
            HIP_TRY(launch_exclusive_scan(h->zs.seq_tot.p, h->zs.seq_base.p, (int64_t)n, h->scan_tmp.p, st));
            h->zs.lit.ensure((size_t)totals[0] + 16);
            h->zs.seq.ensure((size_t)totals[1] + 1);
            mark(2);
            // stages 4, 5; (sync: the output is sized)
            HIP_TRY(launch_zs_decode(d_zst, h->zs.frames.p, h->zs.blocks.p, nb, h->zs.lit_base.p, h->zs.seq_base.p,
                                     h->zs.lit.p, h->zs.seq.p, st));
            mark(3);
            HIP_TRY(launch_zs_chain(h->zs.frames.p, h->zs.blocks.p, n_frames, h->inf.size.p, h->zs.totals.p, st));
            HIP_TRY(hipMemcpyAsync(totals + 2, h->zs.totals.p + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        const unsigned long long total = totals[2];
        if (total >= (1ull << 32) - 64) return fail(SDL_ERR_CAPACITY, "zstd frames decode to >= 4 GiB in one call");
        h->inf.out.ensure((size_t)total + 48);
        HIP_TRY(hipMemsetAsync(h->inf.out.p + total, 0, 32, st));
        uint32_t bad[2] = {0, 0xFFFFFFFFu};
        if (n) {
            HIP_TRY(launch_exclusive_scan(h->inf.size.p, h->inf.off.p, (int64_t)n, h->scan_tmp.p, st));
            HIP_TRY(hipMemcpyAsync(h->inf.bad.p, bad, sizeof(bad), hipMemcpyHostToDevice, st));
            mark(4);
            // stages 6, 7, 8
            HIP_TRY(launch_zs_write(d_zst, h->zs.frames.p, h->zs.blocks.p, nb, n_frames, h->zs.lit_base.p,
                                    h->zs.seq_base.p, h->zs.lit.p, h->zs.seq.p, h->inf.off.p, h->inf.out.p,
                                    !(flags & SDL_ZSTD_NO_CHECKSUM), h->inf.status.p, h->inf.bad.p, st,
                                    h->profiling ? h->ev + 5 : nullptr));
            mark(7);
            HIP_TRY(hipMemcpyAsync(bad, h->inf.bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        } else {
            for (int i = 1; i <= kStages; ++i) mark(i);
            HIP_TRY(hipMemsetAsync(h->inf.off.p, 0, sizeof(uint32_t), st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        std::memset(out, 0, sizeof(*out));
        out->d_out = h->inf.out.p;
        out->d_member_out = h->inf.off.p;
        out->d_status = h->inf.status.p;
        out->out_bytes = total;
        out->n_members = n_frames;
        out->n_bad = bad[0];
        if (bad[0]) {
            int32_t s = 0;
            HIP_TRY(hipMemcpy(&s, h->inf.status.p + bad[1], sizeof(s), hipMemcpyDeviceToHost));
            return fail(SDL_ERR_DATA, "zstd frame " + std::to_string(bad[1]) + ": " + zs_reason(s) + " (" +
                                          std::to_string(bad[0]) + " of " + std::to_string(n_frames) + " frames failed)");
        }
        return SDL_OK;
    });
}

int sdl_zstd_split_frames(const uint8_t *zst, uint64_t len, uint64_t *offsets, uint64_t cap, uint64_t *n_frames) {
    if ((!zst && len) || !n_frames) return fail(SDL_ERR_ARG, "null argument");
    std::vector<uint64_t> off{0};
    while (off.back() < len) {
        zs::FrameInfo fi;
        uint64_t bytes = 0;
        uint32_t nb = 0;
        const int32_t st = zs::frame_extent(zst + off.back(), len - off.back(), fi, bytes, nb);
        if (st) {
            *n_frames = off.size() - 1;
            return fail(SDL_ERR_DATA, "no zstd frame at byte " + std::to_string(off.back()) + ": " + zs_reason(st));
        }
        off.push_back(off.back() + bytes);
    }
    *n_frames = off.size() - 1;
    if (!offsets || cap < off.size()) return fail(SDL_ERR_CAPACITY, "offsets needs n_frames + 1 entries");
    std::memcpy(offsets, off.data(), off.size() * sizeof(uint64_t));
    return SDL_OK;
}
}  // extern "C"
