// provider_json.cpp -- the Provider's JsonText step on the device (json_text.hip).  Its buffers are
// the handle's JsonWork; it borrows the handle's stream, scan_tmp and pin_u32_2.
#include "handle.hpp"

extern "C" {
int sdl_json_text_device(sdl_batcher *h, const uint8_t *d_jsonl, uint64_t len, void *stream, sdl_json_text *out) {
    if (!h || !out || (!d_jsonl && len)) return fail(SDL_ERR_ARG, "null argument");
    if (len >= (1ull << 32)) return fail(SDL_ERR_CAPACITY, "JSON buffer must be < 4 GiB per call");
    if (((uintptr_t)d_jsonl & 15u) != 0) return fail(SDL_ERR_ARG, "d_jsonl must be 16-byte aligned");
    return guarded(SDL_ERR_ARG, SDL_ERR_ARG, [&]() -> int {
        hipStream_t st = stream ? (hipStream_t)stream : h->stream;
        const int64_t N = (int64_t)len, nb = (N + CHUNK - 1) / CHUNK;
        h->json.cnt.ensure((size_t)nb + 1);
        h->json.base.ensure((size_t)nb + 1);
        h->scan_tmp.ensure((size_t)scan_tmp_words(std::max<int64_t>(nb, 1)) + 1);
        // the newline list is sized for JSON lines of >= 64 B on average (a record line is
        // {"text": ...} plus the dump's fields), so the count and the last position come back
        // together in one synchronisation; denser input grows the list and writes it again
        uint32_t n_nl = 0, last_nl = 0;
        const size_t nl_want = std::min<size_t>((size_t)N / 64 + 4096, (size_t)N + 2);
        h->json.nl.ensure(nl_want);
        h->json.tail.ensure(2);
        if (nb) {
            const uint32_t cap = (uint32_t)std::min<size_t>(h->json.nl.cap, 0xFFFFFFFFu);
            HIP_TRY(launch_json_nl_count(d_jsonl, N, h->json.cnt.p, h->json.base.p, h->scan_tmp.p, st));
            HIP_TRY(launch_json_nl_write(d_jsonl, N, h->json.base.p, h->json.nl.p, cap, st));
            HIP_TRY(launch_json_nl_tail(h->json.base.p + nb, h->json.nl.p, cap, h->json.tail.p, st));
            HIP_TRY(hipMemcpyAsync(h->pin_u32_2, h->json.tail.p, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            n_nl = h->pin_u32_2[0];
            last_nl = h->pin_u32_2[1];
            if (n_nl > cap) {  // more lines than the list held: grow it to the count, write again
                h->json.nl.ensure((size_t)n_nl + 2);
                const uint32_t cap2 = (uint32_t)std::min<size_t>(h->json.nl.cap, 0xFFFFFFFFu);
                HIP_TRY(launch_json_nl_write(d_jsonl, N, h->json.base.p, h->json.nl.p, cap2, st));
                HIP_TRY(launch_json_nl_tail(h->json.base.p + nb, h->json.nl.p, cap2, h->json.tail.p, st));
                HIP_TRY(hipMemcpyAsync(h->pin_u32_2, h->json.tail.p, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                last_nl = h->pin_u32_2[1];
            }
        }
        // tokio lines(): a last line without '\n' counts, an empty tail does not
        const int64_t tail0 = n_nl ? (int64_t)last_nl + 1 : 0;
        const int64_t n_lines = (int64_t)n_nl + (N > tail0 ? 1 : 0);
        const size_t L1 = (size_t)n_lines + 1;
        h->json.len.ensure(L1);
        h->json.rec.ensure(L1);
        h->json.toff.ensure(L1);
        h->json.ridx.ensure(L1);
        h->json.span.ensure(L1);
        h->json.off.ensure(L1);
        h->json.inv.ensure(1);
        h->json.text.ensure((size_t)N + 32);
        h->scan_tmp.ensure((size_t)scan_tmp_words(std::max<int64_t>(std::max<int64_t>(nb, n_lines), 1)) + 1);
        HIP_TRY(hipMemsetAsync(h->json.inv.p, 0, 4, st));
        HIP_TRY(hipMemsetAsync(h->json.off.p, 0, 8, st));
        HIP_TRY(launch_json_parse(d_jsonl, N, h->json.nl.p, n_nl, n_lines, h->json.len.p, h->json.rec.p, h->json.span.p,
                                  h->json.inv.p, st));
        uint32_t counts[3] = {0, 0, 0};  // records, text bytes, invalid lines
        if (n_lines) {
            HIP_TRY(launch_exclusive_scan(h->json.len.p, h->json.toff.p, n_lines, h->scan_tmp.p, st));
            HIP_TRY(launch_exclusive_scan(h->json.rec.p, h->json.ridx.p, n_lines, h->scan_tmp.p, st));
            HIP_TRY(launch_json_write(d_jsonl, N, h->json.nl.p, n_nl, n_lines, h->json.rec.p, h->json.span.p, h->json.toff.p, h->json.ridx.p, h->json.text.p,
                                      h->json.off.p, st));
            HIP_TRY(hipMemcpyAsync(&counts[0], h->json.ridx.p + n_lines, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&counts[1], h->json.toff.p + n_lines, 4, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(&counts[2], h->json.inv.p, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemsetAsync(h->json.text.p + counts[1], 0, 16, st));  // zero tail for 16-B readers
        std::memset(out, 0, sizeof(*out));
        out->d_text = h->json.text.p;
        out->d_offsets = h->json.off.p;
        out->n_records = counts[0];
        out->text_bytes = counts[1];
        out->n_lines = (uint64_t)n_lines;
        out->n_invalid = counts[2];
        return SDL_OK;
    });
}
}  // extern "C"
