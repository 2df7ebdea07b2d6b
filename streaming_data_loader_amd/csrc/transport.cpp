// transport.cpp -- the Transport's serde_pickle frames on the device (transport_frame.hip), the
// end-to-end path host JSON lines -> frames that strings the steps together through the C ABI, and
// the D2H helper.  Its buffers are the handle's FrameWork and JsonFramesWork.
#include "handle.hpp"

namespace {

struct FramePlaneDesc {
    const char *name;
    const void *src;
    uint32_t width;
    bool f32;
    bool filled_rows_only;  // BertData.label: one entry per filled row
    bool flat;              // Vec<u32> (SingleClass `label`): one list of B (filled) items
};

// list of `n` items of `item` bytes each: "](" items ["e(" per 1000] "e", or "]" when empty
uint64_t list_bytes(uint64_t n, uint64_t item) { return n ? 3 + n * item + 2 * (n / 1000) : 1; }

// lays out one frame (the plane_rows rows of each plane); returns its size
uint64_t frame_layout(FrameParams &fp, const FramePlaneDesc *d, int np, const uint32_t *plane_rows, bool last) {
    uint64_t pos = 4;  // PROTO 3, EMPTY_DICT, MARK
    for (int p = 0; p < np; ++p) {
        FramePlane &P = fp.plane[p];
        const uint32_t n = (uint32_t)std::strlen(d[p].name);
        P.key_len = 5 + n + (P.flat ? 0 : 2);
        P.key[0] = 'X';
        for (int i = 0; i < 4; ++i) P.key[1 + i] = (uint8_t)(n >> (8 * i));
        std::memcpy(P.key + 5, d[p].name, n);
        if (!P.flat) {
            P.key[5 + n] = ']';
            P.key[6 + n] = '(';
        }
        (last ? P.off_last : P.off_full) = pos + P.key_len;
        pos += 5 + n + (P.flat ? (last ? P.row_bytes_last : P.row_bytes) : list_bytes(plane_rows[p], P.row_bytes));
    }
    return pos + 2;  // SETITEMS, STOP
}

}  // namespace

extern "C" {
int sdl_pickle_frames_device(sdl_batcher *h, const sdl_device_rows *rows, uint64_t n_rows, int flush_partial,
                             void *stream, sdl_frames *out) {
    if (!h || !rows || !out) return fail(SDL_ERR_ARG, "null argument");
    const int task = h->cfg.task;
    const uint64_t B = (uint64_t)h->cfg.batch_size, S = (uint64_t)h->cfg.sequence_length;
    const uint64_t LW = (uint64_t)rows->label_width;
    if (B == 0 || S == 0) return fail(SDL_ERR_ARG, "batch_size and sequence_length must be > 0");
    const uint64_t rem = n_rows % B, n_frames = n_rows / B + (flush_partial && rem ? 1 : 0);
    if (n_frames * B > rows->rows_capacity)
        return fail(SDL_ERR_ARG, "n_rows exceeds the rows the device planes hold");
    const bool bert = task == SDL_TASK_MLM || task == SDL_TASK_MULTI_LABEL || task == SDL_TASK_SINGLE_CLASS;
    FramePlaneDesc d[5];
    int np = 0;
    d[np++] = {"input_ids", rows->input_ids, (uint32_t)S, false, false, false};
    d[np++] = {"attention_mask", rows->attention_mask, (uint32_t)S, false, false, false};
    if (bert) d[np++] = {"token_type_ids", rows->token_type_ids, (uint32_t)S, false, false, false};
    if (task == SDL_TASK_MULTI_LABEL)
        d[np++] = {"labels", rows->labels_f32, (uint32_t)LW, true, true, false};
    else if (task == SDL_TASK_SINGLE_CLASS)  // bert_data.rs:118-121: "label": Vec<u32>
        d[np++] = {"label", rows->labels, 1, false, true, true};
    else
        d[np++] = {"labels", rows->labels, (uint32_t)LW, false, bert, false};
    // mlm sentence pairs: the pair labels of the frame's filled rows, one flat list (like `label`)
    if (h->pair_mlm())
        d[np++] = {h->cfg.pair == SDL_PAIR_MLM_SOP ? "sentence_order_label" : "next_sentence_label",
                   h->pair_lab_ran ? h->o_pair_lab.p : nullptr, 1, false, true, true};
    for (int p = 0; p < np; ++p)
        if (!d[p].src && n_frames) return fail(SDL_ERR_ARG, std::string("device plane missing: ") + d[p].name);
    return guarded(SDL_ERR_ARG, SDL_ERR_ARG, [&]() -> int {
        FrameParams fp{};
        fp.n_planes = np;
        fp.B = (uint32_t)B;
        fp.n_frames = n_frames;
        uint32_t full_rows[5], last_rows[5];
        const bool partial = n_frames && n_frames * B > n_rows;
        for (int p = 0; p < np; ++p) {
            FramePlane &P = fp.plane[p];
            const uint32_t ew = d[p].f32 ? 9 : 5;
            const uint64_t filled_last = partial && d[p].filled_rows_only ? rem : B;
            P.src = d[p].src;
            P.is_f32 = d[p].f32;
            P.flat = d[p].flat;
            if (P.flat) {  // one list per frame of the B (last: filled) values
                P.width = (uint32_t)B;
                P.width_last = (uint32_t)filled_last;
                P.frame_stride = B;
                full_rows[p] = P.rows_full = 1;
                last_rows[p] = P.rows_last = 1;
            } else {
                P.width = P.width_last = d[p].width;
                P.frame_stride = B * d[p].width;
                full_rows[p] = P.rows_full = (uint32_t)B;
                last_rows[p] = P.rows_last = (uint32_t)filled_last;
            }
            P.row_bytes = (uint32_t)list_bytes(P.width, ew);
            P.row_bytes_last = (uint32_t)list_bytes(P.width_last, ew);
        }
        fp.frame_bytes = frame_layout(fp, d, np, full_rows, false);
        fp.last_frame_bytes = frame_layout(fp, d, np, last_rows, true);
        const uint64_t total = n_frames ? (n_frames - 1) * fp.frame_bytes + fp.last_frame_bytes : 0;
        uint8_t *dst = nullptr;
        if (h->frames.dest) {
            if (!h->frames.dry && (size_t)total > h->frames.dest_cap) return fail(SDL_ERR_CAPACITY, "frames exceed the destination");
            dst = h->frames.dest;
        } else if (!h->frames.dry) {
            DevBuf<uint8_t> &fo = *h->frames.target;
            fo.ensure((size_t)total + 16);
            dst = fo.p;
        }
        fp.out = dst;
        hipStream_t st = stream ? (hipStream_t)stream : h->stream;
        if (!h->frames.dry && n_frames) HIP_TRY(launch_frames(fp, st));
        std::memset(out, 0, sizeof(*out));
        out->d_frames = dst;
        out->n_frames = n_frames;
        out->frame_bytes = fp.frame_bytes;
        out->last_frame_bytes = n_frames ? fp.last_frame_bytes : 0;
        out->total_bytes = total;
        return SDL_OK;
    });
}

// ---- End to end, host to host (north_star's path) ------------------------------
// Host JSON lines -> H2D -> JsonText -> tokenize + mask -> serde_pickle frames ->
// D2H -> sink, in chunks cut at line ends, on three streams: chunk k's frames
// copy out (x_out) while chunk k + 1 is copied in (x_in) and computed (the
// handle's stream).  Rows short of a batch at the end of a chunk are carried
// (device to device) to the front of the next chunk's rows, so the frames are
// exactly those of the whole buffer in one call: every full batch, then the
// flushed partial one when flush_partial.  Record indices (RNG keys) continue
// across chunks from cfg.first_record.
int sdl_json_to_frames(sdl_batcher *h, const uint8_t *jsonl, uint64_t len, uint64_t chunk_bytes, int flush_partial,
                       sdl_frame_sink sink, void *user, sdl_json_frames_stats *stats) {
    if (!h || (!jsonl && len)) return fail(SDL_ERR_ARG, "null argument");
    const int task = h->cfg.task;
    if (h->pair_mlm())
        return fail(SDL_ERR_UNSUPPORTED, "sdl_json_to_frames: pair = 2..4 is not supported (one text member a line)");
    if (h->pair())
        return fail(SDL_ERR_UNSUPPORTED, "sdl_json_to_frames: pair = 1 is not supported (one text member a line)");
    if (task != SDL_TASK_MLM && task != SDL_TASK_CLM && task != SDL_TASK_SPAN)
        return fail(SDL_ERR_UNSUPPORTED, "sdl_json_to_frames: JSON lines carry text only (mlm, clm, span)");
    if (h->pack())
        return fail(SDL_ERR_UNSUPPORTED,
                    "sdl_json_to_frames: pack = 1 is not supported (the rows carried between chunks would need "
                    "the id carry too)");
    if (chunk_bytes == 0) chunk_bytes = (uint64_t)8 << 20;
    if (chunk_bytes >= (1ull << 31)) return fail(SDL_ERR_CAPACITY, "chunk_bytes must be < 2 GiB");
    return guarded(SDL_ERR_CAPACITY, SDL_ERR_ARG, [&]() -> int {
        const auto t_start = std::chrono::steady_clock::now();
        if (!h->jf.in) HIP_TRY(hipStreamCreateWithFlags(&h->jf.in, hipStreamNonBlocking));
        if (!h->jf.out) HIP_TRY(hipStreamCreateWithFlags(&h->jf.out, hipStreamNonBlocking));
        for (auto &e : h->jf.ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        // per slot (chunk k uses slot k & 1): H2D done, rows of the chunk ready, frames written
        hipEvent_t *e_h2d = h->jf.ev, *e_rows = h->jf.ev + 2, *e_frames = h->jf.ev + 4;
        const hipStream_t sc = h->stream;
        const uint64_t B = (uint64_t)h->cfg.batch_size, S = (uint64_t)h->cfg.sequence_length;
        const uint64_t LW = (uint64_t)h->P.label_width;
        const bool tt = h->with_tt();
        // chunks end at a '\n' (the last one at len); the first is a quarter chunk so the
        // copy-out stream starts early
        std::vector<uint64_t> cut{0};
        constexpr int64_t head_div = 4;
        while (cut.back() < len) {
            uint64_t e = cut.back() + (cut.size() == 1 ? std::max<uint64_t>(chunk_bytes / head_div, 4096) : chunk_bytes);
            if (e >= len) { cut.push_back(len); break; }
            const void *nl = std::memchr(jsonl + e, '\n', (size_t)(len - e));
            cut.push_back(nl ? (uint64_t)((const uint8_t *)nl - jsonl) + 1 : len);
        }
        const size_t nch = cut.size() - 1;
        // pinned input is copied in directly; pageable input is staged through pinned slots
        bool pinned_in = false;
        {
            hipPointerAttribute_t pa;
            if (len && hipPointerGetAttributes(&pa, jsonl) == hipSuccess && pa.type == hipMemoryTypeHost)
                pinned_in = true;
            (void)hipGetLastError();
        }
        // pinned input: every chunk's H2D is queued up front (one copy each, into its own region
        // followed by 32 zero bytes), so no chunk's input waits behind an earlier chunk's D2H
        std::vector<uint64_t> region(nch + 1, 0);
        for (size_t k = 0; k < nch; ++k) region[k + 1] = region[k] + ((cut[k + 1] - cut[k] + 32 + 255) & ~(uint64_t)255);
        if (pinned_in && nch) {
            while (h->jf.in_ev.size() < nch) {
                hipEvent_t e;
                HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                h->jf.in_ev.push_back(e);
            }
            h->jf.json_all.ensure((size_t)region[nch]);
            HIP_TRY(hipMemsetAsync(h->jf.json_all.p, 0, (size_t)region[nch], h->jf.in));
            for (size_t k = 0; k < nch; ++k) {
                HIP_TRY(hipMemcpyAsync(h->jf.json_all.p + region[k], jsonl + cut[k], (size_t)(cut[k + 1] - cut[k]),
                                       hipMemcpyHostToDevice, h->jf.in));
                HIP_TRY(hipEventRecord(h->jf.in_ev[k], h->jf.in));
            }
        }
        uint64_t carry = 0, carry_at = 0, records = 0, lines = 0, invalid = 0, frames_total = 0, bytes_total = 0;
        uint64_t rows_total = 0, text_total = 0;
        struct Pending {
            bool live = false;
            uint64_t n_frames = 0, frame_bytes = 0, last_bytes = 0, total = 0;
        } pend[2];
        bool used[2] = {false, false};
        double hw[4] = {0, 0, 0, 0};
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto since = [&](std::chrono::steady_clock::time_point t) {
            return std::chrono::duration<double>(now() - t).count();
        };
        auto deliver = [&](int slot) -> int {  // frames of the chunk in slot, once written to host memory
            Pending &q = pend[slot];
            if (!q.live) return 0;
            const auto t0 = now();
            HIP_TRY(hipEventSynchronize(e_frames[slot]));
            hw[3] += since(t0);
            const uint8_t *f = h->jf.pin_out[slot].p;
            for (uint64_t i = 0; i < q.n_frames; ++i) {
                const uint64_t nb = i + 1 == q.n_frames ? q.last_bytes : q.frame_bytes;
                if (sink && sink(user, f, nb) != 0) return fail(SDL_ERR_STATE, "sdl_json_to_frames: sink stopped");
                f += nb;
            }
            q.live = false;
            return 0;
        };
        for (size_t k = 0; k <= nch; ++k) {
            const bool last = k == nch;  // the final pass only flushes the carried rows
            const int slot = (int)(k & 1);
            const uint64_t a = last ? len : cut[k], n = last ? 0 : cut[k + 1] - cut[k];
            // this slot's previous frames (chunk k - 2) leave first: its buffers are reused
            if (int rc = deliver(slot)) return rc;
            uint64_t G = 0;
            sdl_device_rows rows{};
            if (n) {
                const uint8_t *d_json;
                if (pinned_in) {
                    d_json = h->jf.json_all.p + region[k];
                    HIP_TRY(hipStreamWaitEvent(sc, h->jf.in_ev[k], 0));
                } else {
                    h->jf.json[slot].ensure((size_t)n + 32);
                    if (used[slot]) HIP_TRY(hipEventSynchronize(e_h2d[slot]));
                    h->jf.pin_in[slot].ensure((size_t)n + 32);
                    par_copy(h->jf.pin_in[slot].p, jsonl + a, (size_t)n);
                    std::memset(h->jf.pin_in[slot].p + n, 0, 32);
                    HIP_TRY(hipMemcpyAsync(h->jf.json[slot].p, h->jf.pin_in[slot].p, (size_t)n + 32,
                                           hipMemcpyHostToDevice, h->jf.in));
                    HIP_TRY(hipEventRecord(e_h2d[slot], h->jf.in));
                    used[slot] = true;
                    HIP_TRY(hipStreamWaitEvent(sc, e_h2d[slot], 0));
                    d_json = h->jf.json[slot].p;
                }
                sdl_json_text jt;
                auto t0 = now();
                if (int rc = sdl_json_text_device(h, d_json, n, sc, &jt)) return rc;  // syncs sc
                hw[0] += since(t0);
                t0 = now();
                lines += jt.n_lines;
                invalid += jt.n_invalid;
                text_total += jt.text_bytes;
                if (int rc = sdl_process_device(h, jt.d_text, jt.text_bytes, jt.d_offsets, jt.n_records,
                                                h->cfg.first_record + records, sc, &rows))
                    return rc;
                records += jt.n_records;
                uint32_t g32 = 0;
                h->pin_u32_err = 0;
                HIP_TRY(hipMemcpyAsync(&g32, rows.d_rows, 4, hipMemcpyDeviceToHost, sc));
                if (rows.d_tokenize_errors)
                    HIP_TRY(hipMemcpyAsync(&h->pin_u32_err, rows.d_tokenize_errors, 4, hipMemcpyDeviceToHost, sc));
                HIP_TRY(hipStreamSynchronize(sc));
                hw[1] += since(t0);
                if (h->pin_u32_err)
                    throw CapacityError("tokenizer capacity exceeded (d_tokenize_errors flags " +
                                        std::to_string(h->pin_u32_err) + ")");
                G = g32;
            }
            // this pass's rows in its slot's planes: the carried rows (from the other slot), then the chunk's
            const uint64_t have = carry + G;
            const uint64_t cap = have + B;
            h->jf.ids[slot].ensure((size_t)(cap * S));
            h->jf.am[slot].ensure((size_t)(cap * S));
            if (tt) h->jf.tt[slot].ensure((size_t)(cap * S));
            h->jf.lab[slot].ensure((size_t)(cap * LW));
            const int o = slot ^ 1;
            if (carry) {
                HIP_TRY(hipMemcpyAsync(h->jf.ids[slot].p, h->jf.ids[o].p + carry_at * S, carry * S * 4,
                                       hipMemcpyDeviceToDevice, sc));
                HIP_TRY(hipMemcpyAsync(h->jf.am[slot].p, h->jf.am[o].p + carry_at * S, carry * S * 4,
                                       hipMemcpyDeviceToDevice, sc));
                if (tt)
                    HIP_TRY(hipMemcpyAsync(h->jf.tt[slot].p, h->jf.tt[o].p + carry_at * S, carry * S * 4,
                                           hipMemcpyDeviceToDevice, sc));
                HIP_TRY(hipMemcpyAsync(h->jf.lab[slot].p, h->jf.lab[o].p + carry_at * LW, carry * LW * 4,
                                       hipMemcpyDeviceToDevice, sc));
            }
            if (G) {
                HIP_TRY(hipMemcpyAsync(h->jf.ids[slot].p + carry * S, rows.input_ids, G * S * 4, hipMemcpyDeviceToDevice,
                                       sc));
                HIP_TRY(hipMemcpyAsync(h->jf.am[slot].p + carry * S, rows.attention_mask, G * S * 4,
                                       hipMemcpyDeviceToDevice, sc));
                if (tt)
                    HIP_TRY(hipMemcpyAsync(h->jf.tt[slot].p + carry * S, rows.token_type_ids, G * S * 4,
                                           hipMemcpyDeviceToDevice, sc));
                HIP_TRY(hipMemcpyAsync(h->jf.lab[slot].p + carry * LW, rows.labels, G * LW * 4, hipMemcpyDeviceToDevice,
                                       sc));
            }
            rows_total += G;
            uint64_t nframe_rows = have / B * B;
            const bool flush_now = last && flush_partial && have % B;
            if (flush_now) {  // the partial batch: initial values past its rows
                const uint64_t r0 = have, r1 = (have / B + 1) * B;
                HIP_TRY(hipMemsetD32Async(h->jf.ids[slot].p + r0 * S, 0, (r1 - r0) * S, sc));
                HIP_TRY(hipMemsetD32Async(h->jf.am[slot].p + r0 * S, 1, (r1 - r0) * S, sc));
                if (tt) HIP_TRY(hipMemsetD32Async(h->jf.tt[slot].p + r0 * S, 0, (r1 - r0) * S, sc));
                HIP_TRY(hipMemsetD32Async(h->jf.lab[slot].p + r0 * LW, -100, (r1 - r0) * LW, sc));
                nframe_rows = have;
            }
            HIP_TRY(hipEventRecord(e_rows[slot], sc));
            if (nframe_rows) {
                const auto t2 = now();
                sdl_device_rows x{};
                x.input_ids = h->jf.ids[slot].p;
                x.attention_mask = h->jf.am[slot].p;
                x.token_type_ids = tt ? h->jf.tt[slot].p : nullptr;
                x.labels = h->jf.lab[slot].p;
                x.rows_capacity = (have / B + 1) * B;
                x.label_width = (int32_t)LW;
                // size the frames, write them into this slot's device buffer from the copy-out
                // stream and copy them to pinned host memory there: the next chunk's kernels
                // overlap the copy.  (Writing mapped pinned host memory from the kernel itself
                // measured ~25 GB/s of shader stores over PCIe against ~56 GB/s for the DMA copy.)
                // The frames kernel runs on the compute stream, so the copy-out stream holds
                // nothing but the copies and they run back to back.
                sdl_frames fr;
                h->frames.dry = true;
                int rc = sdl_pickle_frames_device(h, &x, nframe_rows, flush_now ? 1 : 0, h->jf.out, &fr);
                h->frames.dry = false;
                if (rc) return rc;
                h->jf.pin_out[slot].ensure((size_t)fr.total_bytes + 16);
                h->jf.frames[slot].ensure((size_t)fr.total_bytes + 16);
                h->frames.dest = h->jf.frames[slot].p;
                h->frames.dest_cap = h->jf.frames[slot].cap;
                rc = sdl_pickle_frames_device(h, &x, nframe_rows, flush_now ? 1 : 0, sc, &fr);
                h->frames.dest = nullptr;
                h->frames.dest_cap = 0;
                if (rc) return rc;
                HIP_TRY(hipEventRecord(e_rows[slot], sc));  // frames written
                HIP_TRY(hipStreamWaitEvent(h->jf.out, e_rows[slot], 0));
                HIP_TRY(hipMemcpyAsync(h->jf.pin_out[slot].p, h->jf.frames[slot].p, (size_t)fr.total_bytes,
                                       hipMemcpyDeviceToHost, h->jf.out));
                HIP_TRY(hipEventRecord(e_frames[slot], h->jf.out));
                pend[slot] = Pending{true, fr.n_frames, fr.frame_bytes, fr.last_frame_bytes, fr.total_bytes};
                frames_total += fr.n_frames;
                bytes_total += fr.total_bytes;
                hw[2] += since(t2);
            }
            // rows short of a batch are carried into the next pass (copied from this slot)
            const uint64_t rem = have - have / B * B;
            carry = last ? 0 : rem;
            carry_at = have - rem;
            // hand over the previous chunk's frames while this one's are written
            if (int rc = deliver(slot ^ 1)) return rc;
        }
        for (int sl = 0; sl < 2; ++sl)
            if (int rc = deliver(sl)) return rc;
        if (stats) {
            std::memset(stats, 0, sizeof(*stats));
            stats->n_lines = lines;
            stats->n_invalid = invalid;
            stats->n_records = records;
            stats->text_bytes = text_total;
            stats->n_rows = rows_total;
            stats->n_frames = frames_total;
            stats->frame_bytes = bytes_total;
            stats->n_chunks = nch;
            stats->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
            for (int i = 0; i < 4; ++i) stats->host_wait[i] = hw[i];
        }
        return SDL_OK;
    });
}

int sdl_device_to_host(sdl_batcher *h, void *dst, const void *src, size_t bytes, void *stream) {
    if (!h || (bytes && (!dst || !src))) return fail(SDL_ERR_ARG, "null argument");
    if (!bytes) return SDL_OK;
    hipStream_t st = stream ? (hipStream_t)stream : h->stream;
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(SDL_ERR_HIP, std::string("sdl_device_to_host: ") + hipGetErrorString(e));
    return SDL_OK;
}
}  // extern "C"
