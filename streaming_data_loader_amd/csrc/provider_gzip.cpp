// provider_gzip.cpp -- the Provider's gzip step on the device (inflate.hip): members one wave each,
// a large member in chunks.  Its buffers are the handle's InflateWork and InflateChunkWork, its
// output the InflatedOut it shares with provider_zstd.cpp; it borrows the handle's stream and scan_tmp.
#include "handle.hpp"

namespace {

const char *gz_reason(int32_t s) {
    static const char *names[] = {"ok",
                                  "member range outside the buffer",
                                  "truncated",
                                  "not a gzip header (magic, method or reserved flags)",
                                  "header crc mismatch",
                                  "invalid block type",
                                  "invalid stored block lengths",
                                  "invalid code lengths set",
                                  "invalid literal/length or distance code",
                                  "invalid distance too far back",
                                  "more output than the trailer's size",
                                  "incorrect length check",
                                  "bytes after the member's trailer",
                                  "incorrect data check",
                                  "decoder made no progress"};
    return s >= 0 && s < (int32_t)(sizeof(names) / sizeof(names[0])) ? names[s] : "unknown";
}

X2N make_x2n() {  // zlib's x2n_table: x^(2^k) mod P(x), reflected
    auto mult = [](uint32_t a, uint32_t b) {
        uint32_t m = 1u << 31, p = 0;
        for (;;) {
            if (a & m) {
                p ^= b;
                if ((a & (m - 1)) == 0) break;
            }
            m >>= 1;
            b = b & 1u ? (b >> 1) ^ 0xEDB88320u : b >> 1;
        }
        return p;
    };
    X2N x{};
    uint32_t p = 1u << 30;  // x^1
    x.t[0] = p;
    for (int k = 1; k < 32; ++k) x.t[k] = p = mult(p, p);
    return x;
}

// A gzip member of >= GZ_SPLIT_MIN compressed bytes -- a single-member .json.gz,
// the reference's own input -- is inflated in chunks (kernels.hpp, "chunked
// members"): a header search per chunk, every chunk decoded at once into 16-bit
// slots, each handing over where a later chunk's searched start is a real block
// start (so wrong picks and block starts the search skips -- stored or fixed
// blocks -- are decoded through in the same launch); the host follows the
// hand-overs in stream order and continues a chunk whose slot filled up with a
// new one resuming inside the block (its header parsed again); the window chain,
// bytes, CRC-32 and ISIZE follow on the device.  The member's status gets
// GZ_VERIFIED so the one-wave path skips it.
constexpr uint64_t GZ_SPLIT_MIN = 1u << 20;  // smaller members: one wave each
constexpr uint64_t GZ_CHUNK = 24u << 10;     // compressed bytes per chunk (at least; 16/20/28/32/64 KiB measured slower)
constexpr uint64_t GZ_MAX_CHUNKS = 8192;     // (larger members: larger chunks)
constexpr uint32_t GZ_SLOT_RATIO = 16;       // slot values per compressed byte of a chunk
constexpr uint64_t GZ_FIND_SPAN = 2;         // header search: this many chunk lengths of bits
constexpr uint64_t GZ_EXTRA_CHUNKS = 256;    // chunks appended behind one that stopped for capacity

void inflate_chunked(sdl_batcher *h, const uint8_t *d_gz, uint64_t m, uint64_t ma, uint64_t mz, uint32_t isize,
                     uint32_t ooff_m, hipStream_t st) {
    const uint64_t len = mz - ma;
    uint64_t ch = GZ_CHUNK;
    while ((len + ch - 1) / ch > GZ_MAX_CHUNKS) ch *= 2;
    const uint64_t C0 = (len - 8 + ch - 1) / ch;  // nominal starts ma + c ch < mz - 8
    const uint64_t CT = C0 + GZ_EXTRA_CHUNKS;
    // 16-bit slot values per chunk: GZ_SLOT_RATIO x its compressed bytes, unless the member's
    // slots together would exceed 8x its ISIZE in bytes (~4x the output per chunk on average);
    // a chunk whose slot fills stops at a flush point and is resumed (GZC_SOFT)
    uint64_t cap64 = ch * GZ_SLOT_RATIO;
    const uint64_t slot_budget = std::max<uint64_t>(8ull * isize, 256ull << 20);
    if (CT * cap64 * 2 > slot_budget) cap64 = std::max<uint64_t>(2 * ch, slot_budget / (2 * CT));
    const uint32_t cap = (uint32_t)cap64;
    static const bool dbg = std::getenv("SDL_GZ_DEBUG") != nullptr;  // diagnostic: phase times to stderr
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms_since = [&](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(now() - t).count();
    };
    const auto t_begin = now();
    int redos = 0;
    try {  // device memory for the chunked path; without it the one-wave path decodes the member
    h->gzc.nominal.ensure(CT);
    h->gzc.found.ensure(CT);
    h->gzc.start.ensure(CT);
    h->gzc.hdr.ensure(CT);
    h->gzc.end.ensure(CT);
    h->gzc.endhdr.ensure(CT);
    h->gzc.pos.ensure(CT);
    h->gzc.list.ensure(CT);
    h->gzc.tgt.ensure(CT);
    h->gzc.next.ensure(CT);
    h->gzc.len.ensure(CT);
    h->gzc.flags.ensure(CT);
    h->gzc.order.ensure(CT);
    h->gzc.crc.ensure(CT);
    h->gzc.shift.ensure(CT);
    h->gzc.status.ensure(CT);
    h->gzc.rstatus.ensure(1);
    h->gzc.slots.ensure((size_t)CT * cap);
    } catch (const HipError &) {
        (void)hipGetLastError();  // (clear the allocation failure so later launches do not report it)
        return;
    }
    std::vector<uint64_t> nominal(CT, GZ_NO_BIT), start(CT, GZ_NO_BIT), hdr(CT, GZ_NO_BIT), end(CT, 0),
        endhdr(CT, 0);
    std::vector<uint32_t> clen(CT, 0), flags(CT, 0), tgt(CT, 0), next(CT, ~0u);
    std::vector<int32_t> status(CT, GZ_OK);
    nominal[0] = 0;
    for (uint64_t c = 1; c < C0; ++c) nominal[c] = 8 * (ma + c * ch);
    for (uint64_t c = 0; c < C0; ++c) tgt[c] = (uint32_t)(c + 1);
    HIP_TRY(hipMemcpyAsync(h->gzc.nominal.p, nominal.data(), C0 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->gzc.tgt.p, tgt.data(), C0 * 4, hipMemcpyHostToDevice, st));
    if (dbg) {
        h->gzc.stats.ensure(3 * C0);
        HIP_TRY(hipMemsetAsync(h->gzc.stats.p, 0, 3 * C0 * 4, st));
    }
    if (C0 > 1)
        HIP_TRY(launch_gz_find(d_gz, ma, mz, h->gzc.nominal.p + 1, C0 - 1, 8 * GZ_FIND_SPAN * ch, h->gzc.found.p + 1,
                               dbg ? h->gzc.stats.p : nullptr, st));
    HIP_TRY(hipMemcpyAsync(start.data() + 1, h->gzc.found.p + 1, (C0 - 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double t_find = ms_since(t_begin);
    if (dbg && C0 > 1) {
        std::vector<uint32_t> sv(3 * (C0 - 1));
        HIP_TRY(hipMemcpy(sv.data(), h->gzc.stats.p, sv.size() * 4, hipMemcpyDeviceToHost));
        double m[4] = {0, 0, 0, 0};
        uint32_t mx[4] = {0, 0, 0, 0};
        uint64_t nf = 0;
        for (uint64_t c = 0; c + 1 < C0; ++c) {
            nf += start[c + 1] == GZ_NO_BIT;
            const uint32_t v[4] = {sv[3 * c], sv[3 * c + 1] & 4095u, sv[3 * c + 1] >> 12, sv[3 * c + 2]};
            for (int k = 0; k < 4; ++k) {
                m[k] += v[k];
                mx[k] = std::max(mx[k], v[k]);
            }
        }
        fprintf(stderr, "[gz find] per chunk: stages mean %.1f max %u, full checks mean %.1f max %u, "
                "scan kticks mean %.0f max %u, check kticks mean %.0f max %u; %llu without a start\n",
                m[0] / (C0 - 1), mx[0], m[1] / (C0 - 1), mx[1], m[2] / (C0 - 1), mx[2], m[3] / (C0 - 1), mx[3],
                (unsigned long long)nf);
    }
    start[0] = GZ_START_HEADER;
    for (uint64_t c = 0; c < C0; ++c) hdr[c] = start[c];  // searched starts are block boundaries
    HIP_TRY(hipMemcpyAsync(h->gzc.found.p, start.data(), 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->gzc.start.p, start.data(), C0 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->gzc.hdr.p, hdr.data(), C0 * 8, hipMemcpyHostToDevice, st));
    GzChunkArgs a{};
    a.ma = ma;
    a.mz = mz;
    a.list = h->gzc.list.p;
    a.start_bit = h->gzc.start.p;
    a.hdr_bit = h->gzc.hdr.p;
    a.nominal = h->gzc.nominal.p;
    a.found = h->gzc.found.p;
    a.n_chunks = (uint32_t)C0;
    a.tgt0 = h->gzc.tgt.p;
    a.slots = h->gzc.slots.p;
    a.cap = cap;
    a.end_bit = h->gzc.end.p;
    a.end_hdr = h->gzc.endhdr.p;
    a.next = h->gzc.next.p;
    a.len = h->gzc.len.p;
    a.flags = h->gzc.flags.p;
    a.status = h->gzc.status.p;
    // (i) every chunk with a start, at once
    std::vector<uint32_t> list;
    for (uint64_t c = 0; c < C0; ++c)
        if (start[c] != GZ_NO_BIT) list.push_back((uint32_t)c);
    HIP_TRY(hipMemcpyAsync(h->gzc.list.p, list.data(), list.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(launch_inflate_chunks(d_gz, a, list.size(), st));
    HIP_TRY(hipMemcpyAsync(end.data(), h->gzc.end.p, C0 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(endhdr.data(), h->gzc.endhdr.p, C0 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(next.data(), h->gzc.next.p, C0 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(clen.data(), h->gzc.len.p, C0 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(flags.data(), h->gzc.flags.p, C0 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(status.data(), h->gzc.status.p, C0 * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const double t_decode = ms_since(t_begin);
    // (ii) the hand-overs in stream order; a chunk whose slot filled up is continued
    // by a new chunk from its last flush point
    auto resume_from = [&](uint64_t r, uint64_t from, uint64_t from_hdr) {
        start[r] = from;
        hdr[r] = from_hdr;
        uint32_t d = 1;  // the first searched chunk whose search began past `from`
        while (d < C0 && nominal[d] <= from) ++d;
        tgt[r] = d;
        const uint32_t one = (uint32_t)r;
        HIP_TRY(hipMemcpyAsync(h->gzc.start.p + r, &start[r], 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->gzc.hdr.p + r, &hdr[r], 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->gzc.tgt.p + r, &tgt[r], 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->gzc.list.p, &one, 4, hipMemcpyHostToDevice, st));
        HIP_TRY(launch_inflate_chunks(d_gz, a, 1, st));
        ++redos;
        HIP_TRY(hipMemcpyAsync(&end[r], h->gzc.end.p + r, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&endhdr[r], h->gzc.endhdr.p + r, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&next[r], h->gzc.next.p + r, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&clen[r], h->gzc.len.p + r, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&flags[r], h->gzc.flags.p + r, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&status[r], h->gzc.status.p + r, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    };
    std::vector<uint32_t> order;
    std::vector<uint64_t> pos;
    uint64_t C = C0, total = 0;
    int32_t err = GZ_OK;
    bool done = false;
    for (uint64_t c = 0;;) {
        if (status[c] != GZ_OK) {
            err = status[c];
            break;
        }
        order.push_back((uint32_t)c);
        pos.push_back(total);
        total += clen[c];
        if (flags[c] & GZC_FINAL) {
            done = true;
            break;
        }
        if (flags[c] & GZC_SOFT) {
            if (C >= CT) {
                err = GZ_E_OVER;
                break;
            }
            const uint64_t r = C++;
            resume_from(r, end[c], endhdr[c]);
            c = r;
            continue;
        }
        if (next[c] >= C0) {  // (a chunk stops only at a hand-over, the final block or a full slot)
            err = GZ_E_STALL;
            break;
        }
        c = next[c];
    }
    if (err == GZ_OK && !done) err = GZ_E_TRUNC;
    if (err == GZ_OK) {  // the trailer right behind the final block, and ISIZE
        const uint64_t t = (end[order.back()] + 7) >> 3;
        if (t + 8 > mz) err = GZ_E_TRUNC;
        else if (t + 8 != mz) err = GZ_E_TRAIL;
        else if (total != isize) err = GZ_E_SIZE;
    }
    if (err == GZ_E_OVER || err == GZ_E_STALL) return;  // (chunk slots exhausted: the one-wave path decodes it)
    if (err != GZ_OK) {
        const int32_t v = err | GZ_VERIFIED;
        HIP_TRY(hipMemcpyAsync(h->inf.status.p + m, &v, 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // (v is on this stack)
        return;
    }
    // (iii) window chain, bytes + CRC per chunk, the member's CRC
    const uint64_t no = order.size();
    h->gzc.windows.ensure((size_t)no * 32768);
    const uint64_t ngroups = (no + gz_window_group(no) - 1) / gz_window_group(no);
    h->gzc.gmaps.ensure((size_t)ngroups * 32768);
    h->gzc.gwin.ensure((size_t)ngroups * 32768);
    HIP_TRY(hipMemcpyAsync(h->gzc.order.p, order.data(), no * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->gzc.pos.p, pos.data(), no * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(h->gzc.rstatus.p, 0, 4, st));
    static const X2N x2n = make_x2n();
    const double t_walk = ms_since(t_begin);
    HIP_TRY(launch_gz_windows(h->gzc.slots.p, cap, h->gzc.order.p, h->gzc.len.p, no, h->gzc.windows.p, h->gzc.gmaps.p,
                              h->gzc.gwin.p, st));
    if (dbg) HIP_TRY(hipStreamSynchronize(st));
    const double t_win = ms_since(t_begin);
    HIP_TRY(launch_gz_resolve(h->gzc.slots.p, cap, h->gzc.order.p, h->gzc.len.p, h->gzc.pos.p, no, h->gzc.windows.p,
                              h->inf.out.p + ooff_m, h->gzc.crc.p, h->gzc.shift.p, x2n, h->gzc.rstatus.p, st));
    if (dbg) HIP_TRY(hipStreamSynchronize(st));
    const double t_res = ms_since(t_begin);
    HIP_TRY(launch_gz_crc_fold(h->gzc.crc.p, h->gzc.shift.p, no, d_gz + mz - 8, h->gzc.rstatus.p, h->inf.status.p + m, st));
    HIP_TRY(hipStreamSynchronize(st));  // (order / pos are host vectors)
    if (dbg) {
        int soft = 0;
        for (uint32_t c : order) soft += (flags[c] & GZC_SOFT) != 0;
        fprintf(stderr, "[gz chunked] %llu B member: %llu chunks of %llu B, %zu decoded at once, %d resumed, %llu in "
                "order (%d stopped full); ms: find %.2f decode %.2f walk %.2f windows %.2f resolve %.2f fold %.2f\n",
                (unsigned long long)len, (unsigned long long)C0, (unsigned long long)ch, list.size(), redos,
                (unsigned long long)no, soft, t_find, t_decode - t_find, t_walk - t_decode, t_win - t_walk,
                t_res - t_win, ms_since(t_begin) - t_res);
    }
}

// sdl_gzip_inflate_device, members [d_member_offsets[m], d_member_ends[m]) when d_member_ends is
// given (device, u64[n]; else [offsets[m], offsets[m + 1]))
int gzip_inflate_impl(sdl_batcher *h, const uint8_t *d_gz, uint64_t gz_len, const uint64_t *d_member_offsets,
                      const uint64_t *d_member_ends, uint64_t n_members, void *stream, sdl_inflated *out) {
    if (!h || !out || (n_members && (!d_gz || !d_member_offsets))) return fail(SDL_ERR_ARG, "null argument");
    if (gz_len >= (1ull << 32)) return fail(SDL_ERR_CAPACITY, "gzip buffer must be < 4 GiB per call");
    if (n_members >= (1ull << 31)) return fail(SDL_ERR_CAPACITY, "too many gzip members in one call");
    if (((uintptr_t)d_gz & 15u) != 0) return fail(SDL_ERR_ARG, "d_gz must be 16-byte aligned");
    return guarded(SDL_ERR_ARG, SDL_ERR_ARG, [&]() -> int {
        hipStream_t st = stream ? (hipStream_t)stream : h->stream;
        const size_t n = (size_t)n_members;
        h->inf.size.ensure(n + 1);
        h->inf.off.ensure(n + 1);
        h->gz.tcrc.ensure(n + 1);
        h->inf.status.ensure(n + 1);
        h->gz.total.ensure(1);
        h->inf.bad.ensure(2);
        h->scan_tmp.ensure((size_t)scan_tmp_words(std::max<int64_t>((int64_t)n, 1)) + 1);
        HIP_TRY(hipMemsetAsync(h->gz.total.p, 0, sizeof(unsigned long long), st));
        unsigned long long total = 0;
        if (n) {
            HIP_TRY(launch_gz_size(d_gz, gz_len, d_member_offsets, n_members, h->inf.size.p, h->inf.status.p, h->gz.total.p, st,
                                   d_member_ends));
            HIP_TRY(launch_exclusive_scan(h->inf.size.p, h->inf.off.p, (int64_t)n, h->scan_tmp.p, st));
            HIP_TRY(hipMemcpyAsync(&total, h->gz.total.p, sizeof(total), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        // the trailers' sizes are untrusted until decoded: bound the arena, never the kernel's writes
        if (total >= (1ull << 32) - 64) return fail(SDL_ERR_CAPACITY, "gzip members inflate to >= 4 GiB in one call");
        h->inf.out.ensure((size_t)total + 48);
        HIP_TRY(hipMemsetAsync(h->inf.out.p + total, 0, 32, st));
        uint32_t bad[2] = {0, 0xFFFFFFFFu};
        if (n) {  // large members first, in chunks (they leave GZ_VERIFIED statuses)
            std::vector<uint64_t> mo(n + 1), me(n);
            HIP_TRY(hipMemcpyAsync(mo.data(), d_member_offsets, (d_member_ends ? n : n + 1) * 8, hipMemcpyDeviceToHost, st));
            if (d_member_ends) HIP_TRY(hipMemcpyAsync(me.data(), d_member_ends, n * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (!d_member_ends)
                for (size_t m = 0; m < n; ++m) me[m] = mo[m + 1];
            std::vector<uint64_t> big;
            for (size_t m = 0; m < n; ++m)
                if (me[m] > mo[m] && me[m] - mo[m] >= GZ_SPLIT_MIN && me[m] <= gz_len) big.push_back(m);
            if (!big.empty()) {
                std::vector<uint32_t> sz(n), oo(n);
                std::vector<int32_t> zs(n);
                HIP_TRY(hipMemcpyAsync(sz.data(), h->inf.size.p, n * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(oo.data(), h->inf.off.p, n * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipMemcpyAsync(zs.data(), h->inf.status.p, n * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                for (uint64_t m : big)
                    if (zs[m] == GZ_OK) inflate_chunked(h, d_gz, m, mo[m], me[m], sz[m], oo[m], st);
            }
        }
        if (n) {
            HIP_TRY(hipMemcpyAsync(h->inf.bad.p, bad, sizeof(bad), hipMemcpyHostToDevice, st));
            HIP_TRY(launch_inflate(d_gz, d_member_offsets, n_members, h->inf.off.p, h->inf.out.p, h->inf.status.p, h->gz.tcrc.p, st,
                                   d_member_ends));
            static const X2N x2n = make_x2n();
            HIP_TRY(launch_gz_crc(h->inf.off.p, h->inf.out.p, n_members, h->gz.tcrc.p, x2n, h->inf.status.p, h->inf.bad.p, st));
            HIP_TRY(hipMemcpyAsync(bad, h->inf.bad.p, sizeof(bad), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
#ifdef SDL_STAMPS
            print_gz_cycles();
#endif
        }
        std::memset(out, 0, sizeof(*out));
        out->d_out = h->inf.out.p;
        out->d_member_out = h->inf.off.p;
        out->d_status = h->inf.status.p;
        out->out_bytes = total;
        out->n_members = n_members;
        out->n_bad = bad[0];
        if (bad[0]) {
            int32_t s = 0;
            HIP_TRY(hipMemcpy(&s, h->inf.status.p + bad[1], sizeof(s), hipMemcpyDeviceToHost));
            return fail(SDL_ERR_DATA, "gzip member " + std::to_string(bad[1]) + ": " + gz_reason(s) + " (" +
                                          std::to_string(bad[0]) + " of " + std::to_string(n_members) +
                                          " members failed)");
        }
        return SDL_OK;
    });
}
}  // namespace

extern "C" {
int sdl_gzip_inflate_device(sdl_batcher *h, const uint8_t *d_gz, uint64_t gz_len, const uint64_t *d_member_offsets,
                            uint64_t n_members, void *stream, sdl_inflated *out) {
    return gzip_inflate_impl(h, d_gz, gz_len, d_member_offsets, nullptr, n_members, stream, out);
}

int sdl_gzip_inflate_first_device(sdl_batcher *h, const uint8_t *d_gz, uint64_t gz_len, const uint64_t *d_file_offsets,
                                  uint64_t n_files, void *stream, sdl_inflated *out) {
    if (!h || !out || (n_files && (!d_gz || !d_file_offsets))) return fail(SDL_ERR_ARG, "null argument");
    if (n_files >= (1ull << 31)) return fail(SDL_ERR_CAPACITY, "too many gzip files in one call");
    return guarded(SDL_ERR_ARG, SDL_ERR_ARG, [&]() -> int {
        hipStream_t st = stream ? (hipStream_t)stream : h->stream;
        const size_t n = (size_t)n_files;
        if (n == 0) return gzip_inflate_impl(h, d_gz, gz_len, d_file_offsets, nullptr, 0, stream, out);
        std::vector<uint64_t> fo(n + 1), from(n), ends(n);
        HIP_TRY(hipMemcpyAsync(fo.data(), d_file_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t f = 0; f < n; ++f) {
            if (fo[f + 1] < fo[f] || fo[f + 1] > gz_len) return fail(SDL_ERR_ARG, "file offsets out of order or range");
            from[f] = fo[f] + 19;  // a member is >= 20 bytes: header 10, a final block >= 2, trailer 8
        }
        h->gz.from.ensure(n);
        h->gz.mend.ensure(n);
        // The first member of file f ends at the next offset where a member header could start, or at
        // the file's end.  A candidate inside the member's own DEFLATE data fails its decode (the
        // range ends early); the file then retries from the next candidate.  Every try decodes every
        // file again (such candidates are rare: ~2^-27 per compressed byte).
        for (int attempt = 0;; ++attempt) {
            for (size_t f = 0; f < n; ++f) ends[f] = fo[f + 1];
            HIP_TRY(hipMemcpyAsync(h->gz.from.p, from.data(), n * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(h->gz.mend.p, ends.data(), n * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(launch_gz_next_header(d_gz, gz_len, d_file_offsets, n, h->gz.from.p,
                                          reinterpret_cast<unsigned long long *>(h->gz.mend.p), st));
            HIP_TRY(hipMemcpyAsync(ends.data(), h->gz.mend.p, n * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            const int rc = gzip_inflate_impl(h, d_gz, gz_len, d_file_offsets, h->gz.mend.p, n_files, stream, out);
            if (rc == SDL_ERR_CAPACITY && attempt < 63) {
                // A range that ends at a candidate inside its member's DEFLATE data read its "ISIZE"
                // from 4 arbitrary bytes, which the 1032:1 bound no longer rejects once the range
                // is a few MB: the sizes overflowed the arena.  Advance the candidate-ended files
                // with the largest sizes until the rest fits, and try again (a real first member
                // this large could not be inflated in one call anyway).
                std::vector<uint32_t> sz(n);
                HIP_TRY(hipMemcpy(sz.data(), h->inf.size.p, n * 4, hipMemcpyDeviceToHost));
                unsigned long long tot = 0;
                std::vector<size_t> cand;
                for (size_t f = 0; f < n; ++f) {
                    tot += sz[f];
                    if (ends[f] < fo[f + 1]) cand.push_back(f);
                }
                std::sort(cand.begin(), cand.end(), [&](size_t x, size_t y) { return sz[x] > sz[y]; });
                bool moved = false;
                for (size_t f : cand) {
                    if (tot < (1ull << 32) - 64) break;
                    tot -= sz[f];
                    from[f] = ends[f];
                    moved = true;
                }
                if (moved) continue;
            }
            if (rc != SDL_ERR_DATA || attempt >= 63) return rc;
            std::vector<int32_t> zs(n);
            HIP_TRY(hipMemcpy(zs.data(), h->inf.status.p, n * 4, hipMemcpyDeviceToHost));
            bool again = false;
            for (size_t f = 0; f < n; ++f) {
                const int32_t s = zs[f] & 0xFFFF;
                // a failure that a later end can change: not the header, and not a stream that ended
                // before the range (trailing bytes with no member header: the limit of this mode)
                if (s != GZ_OK && s != GZ_E_HEADER && s != GZ_E_HCRC && s != GZ_E_RANGE && s != GZ_E_TRAIL &&
                    ends[f] < fo[f + 1]) {
                    from[f] = ends[f];
                    again = true;
                }
            }
            if (!again) return rc;
        }
    });
}

int sdl_gzip_split_members(const uint8_t *gz, uint64_t len, uint64_t *offsets, uint64_t cap, uint64_t *n_members) {
    if ((!gz && len) || !n_members) return fail(SDL_ERR_ARG, "null argument");
    // BGZF: FEXTRA with subfield SI1 'B' SI2 'C' SLEN 2 holding the member size - 1
    auto bsize = [&](uint64_t a) -> uint64_t {
        if (a + 18 > len || gz[a] != 0x1f || gz[a + 1] != 0x8b || gz[a + 2] != 8 || !(gz[a + 3] & 4)) return 0;
        const uint64_t xlen = (uint64_t)gz[a + 10] | (uint64_t)gz[a + 11] << 8;
        for (uint64_t q = a + 12; q + 4 <= a + 12 + xlen && q + 4 <= len;) {
            const uint64_t sl = (uint64_t)gz[q + 2] | (uint64_t)gz[q + 3] << 8;
            if (gz[q] == 'B' && gz[q + 1] == 'C' && sl == 2 && q + 6 <= len)
                return ((uint64_t)gz[q + 4] | (uint64_t)gz[q + 5] << 8) + 1;
            q += 4 + sl;
        }
        return 0;
    };
    std::vector<uint64_t> off{0};
    if (len) {
        uint64_t a = 0, b;
        while (a < len && (b = bsize(a)) != 0 && a + b <= len) {
            a += b;
            off.push_back(a);
        }
        if (a < len) {
            if (off.size() > 1) return fail(SDL_ERR_DATA, "BGZF member at byte " + std::to_string(a) + " has no block size");
            off.push_back(len);  // not BGZF: the file is one member
        }
    }
    *n_members = off.size() - 1;
    if (!offsets || cap < off.size()) return fail(SDL_ERR_CAPACITY, "offsets needs n_members + 1 entries");
    std::memcpy(offsets, off.data(), off.size() * sizeof(uint64_t));
    return SDL_OK;
}
}  // extern "C"
