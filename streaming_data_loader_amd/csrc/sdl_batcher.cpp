// sdl_batcher.cpp -- C ABI of the MI355X Batcher (include/sdl_batcher.h).
//
// Host side of the drop-in for the reference's Batcher stage:
//   - sdl_batcher_create  ~ masking_runner::create_generator (masking_runner.rs:55-62)
//                           -> get_tokenizer + GenTokenizer::new (gen_batcher.rs:23-41)
//   - sdl_batcher_push    ~ Batcher::create_sync_batch (gen_batcher.rs:69-94)
//   - sdl_batcher_flush   ~ Batcher::get_working_batch (gen_batcher.rs:96-98)
// The per-record arithmetic runs on the GPU (sdl_process_device); this file
// only moves bytes and keeps GenTokenizer's VecDeque<DataSet> of batches so the
// emission cadence (at most one batch per create_sync_batch call, one flush at
// end of stream) is the reference's.
#include <dlfcn.h>

#include "handle.hpp"
#include "pack_queue.hpp"
#include "span_noise.hpp"

namespace {

// SDL_HOST_TIMING=1: wall-clock split of the host path on stderr (diagnostic)
struct HostClock {
    bool on;
    std::chrono::steady_clock::time_point t;
    std::string s;
    HostClock() : on(std::getenv("SDL_HOST_TIMING") != nullptr), t(std::chrono::steady_clock::now()) {}
    void lap(const char *name) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        s += std::string(" ") + name + "=" +
             std::to_string(std::chrono::duration<double, std::milli>(n - t).count()) + "ms";
        t = n;
    }
    void report(int64_t N, size_t segs, size_t fresh) const {
        if (on)
            fprintf(stderr, "[host] %lld B, %zu segments, %zu pinned blocks so far:%s\n", (long long)N, segs, fresh,
                    s.c_str());
    }
};

// pipelined segments: the tokenize launches, then the downstream work left after the last one
const char *kPipedStageNames[] = {"chunk_ranges", "tokenize", "downstream_tail"};

}  // namespace

const char *sdl::kStageNames[] = {"chunk_ranges", "tokenize", "scan_chunks", "compact_tokens", "records", "scan_rows", "rows"};

PackParams sdl_batcher::pack_params(int64_t R, int64_t rows_cap) {
    const size_t S = (size_t)P.S;
    const int cur = pk_cur, nxt = cur ^ 1;
    PackParams q{};
    q.tok = tok_ids.p;
    q.rec_tok = rec_tok.p;
    q.rec_cnt = rec_cnt.p;
    q.rec_len = rec_rows.p;
    q.pk_off = pk_off.p;
    q.R = R;
    q.rows_cap = rows_cap;
    q.S = P.S;
    q.B = P.B;
    q.eos = tok.eos_id;
    q.min_ids = P.min_ids;
    q.carry_ids = pk_carry.p + (size_t)cur * 2 * S;
    q.carry_pos = q.carry_ids + S;
    q.carry_len = pk_meta.p + 1 + cur;
    q.new_ids = pk_carry.p + (size_t)nxt * 2 * S;
    q.new_pos = q.new_ids + S;
    q.new_len = pk_meta.p + 1 + nxt;
    q.ids = o_ids.p;
    q.am = o_am.p;
    q.lab = o_lab.p;
    q.pos = o_tt.p;
    q.d_rows = pk_meta.p;
    return q;
}
// the call's rows from rec_tok / rec_cnt (after launch_records): packed lengths, their scan
// seeded with the carry length, the gather and the new carry -- no host synchronisation
void sdl_batcher::run_pack(int64_t R, int64_t rows_cap, hipStream_t st) {
    pk_off.ensure((size_t)R + 1);
    const PackParams q = pack_params(R, rows_cap);
    HIP_TRY(launch_pack_lengths(q, st));
    HIP_TRY(launch_exclusive_scan(rec_rows.p, pk_off.p, R, scan_tmp.p, st, pk_off.p));
    HIP_TRY(launch_pack_rows(q, st));
    pk_cur ^= 1;
    pk_ran = true;
}
// the flush row into row 0 of the planes (0 rows when the carry is empty); empties the carry
void sdl_batcher::run_pack_flush(hipStream_t st) {
    const int64_t rows_cap = P.B;
    const size_t plane = (size_t)rows_cap * P.S;
    o_ids.ensure(plane);
    o_am.ensure(plane);
    o_tt.ensure(plane);
    o_lab.ensure(plane);
    HIP_TRY(launch_pack_flush(pack_params(0, rows_cap), st));
    pk_cur ^= 1;
    pk_ran = true;
    last_rows_cap = rows_cap;
    last_R = 0;
}

// pair = 1: the call's rows from rec_tok / rec_cnt of its 2 n text ranges (after launch_records), one
// launch for the three planes, then the task's label kernel over n rows -- no host synchronisation;
// pair 2..4 (mlm): one launch for the four planes and the pair labels (pair_mlm.hip)
void sdl_batcher::run_pair(int64_t R, int64_t rows_cap, int64_t n_chunks, const uint64_t *d_off, uint64_t first_record,
                           hipStream_t st, const uint32_t *d_labels, const uint64_t *d_label_off) {
    const int64_t n = R / 2;
    pair_rb.ensure(2);
    if (pair_mlm()) {
        o_pair_lab.ensure((size_t)std::max<int64_t>(rows_cap, 1));
        PairMlmParams m{};
        m.lists = reinterpret_cast<const uint16_t *>(tokc.p);
        m.chunk_off = chunk_off.p;
        m.off = d_off;
        m.n_lists = n_chunks;
        m.rec_tok = rec_tok.p;
        m.rec_cnt = rec_cnt.p;
        m.n_pairs = n;
        m.rows_end = std::min<int64_t>((n + P.B - 1) / P.B * P.B, rows_cap);
        m.seed = P.seed;
        m.first_record = first_record;
        m.S = P.S;
        m.cls = tok.tpl_cls;
        m.sep = tok.tpl_sep;
        m.mode = cfg.pair;
        m.mask_length = P.mask_length;
        m.mask_id = P.mask_id;
        m.mp = mpol;
        m.ids = o_ids.p;
        m.am = o_am.p;
        m.tt = o_tt.p;
        m.lab = o_lab.p;
        m.pair_lab = o_pair_lab.p;
        m.row_off = row_off.p;
        m.row_rec = row_rec.p;
        m.rb = pair_rb.p;
        HIP_TRY(launch_rows_pair_mlm(m, st));
        pair_lab_ran = true;
        return;
    }
    PairParams q{};
    q.lists = reinterpret_cast<const uint16_t *>(tokc.p);
    q.chunk_off = chunk_off.p;
    q.off = d_off;
    q.n_lists = n_chunks;
    q.rec_tok = rec_tok.p;
    q.rec_cnt = rec_cnt.p;
    q.n_pairs = n;
    q.rows_end = std::min<int64_t>((n + P.B - 1) / P.B * P.B, rows_cap);
    q.S = P.S;
    q.cls = tok.tpl_cls;  // (the loaded BertProcessing's own ids: P.pre / P.post hold the reference's doubled framing)
    q.sep = tok.tpl_sep;
    q.ids = o_ids.p;
    q.am = o_am.p;
    q.tt = o_tt.p;
    q.row_off = row_off.p;
    q.row_rec = row_rec.p;
    q.rb = pair_rb.p;
    HIP_TRY(launch_rows_pair(q, st));
    const SegSel sel{pair_rb.p, 0, 1};
    if (multi())
        HIP_TRY(launch_multi_labels(d_labels, d_label_off, row_rec.p, row_off.p, sel, rows_cap, P.B, P.label_width,
                                    o_f32.p, lab_err.p, st));
    else
        HIP_TRY(launch_single_labels(d_labels, d_label_off, row_rec.p, row_off.p, sel, rows_cap, P.B, o_lab.p,
                                     lab_err.p, st));
}

int64_t sdl_batcher::rows_capacity(int64_t N, int64_t R) const {
    // rows <= sum_r ceil((ids_r + frame) / S) with ids_r <= bytes_r
    const int64_t F = P.n_pre + P.n_post;
    // ids <= bytes (WordPiece, BPE); Unigram: <= 2 * bytes + the pool slack
    const int64_t ids = dt.kind == TOK_UNIGRAM ? 2 * N + 1024 * 1024 : N;
    int64_t cap = P.chunk ? (ids + R * (F + P.S - 1)) / P.S + 1 : R;
    if (pack()) cap = (ids + R + P.S - 1) / P.S + 1;  // the carry (< S) + every id + an eos per record
    if (pair()) cap = R / 2;                          // a row per pair of text ranges
    return (cap + P.B - 1) / P.B * P.B;
}

void sdl_batcher::run_device(const uint8_t *d_text, int64_t N, const uint64_t *d_off, int64_t R, uint64_t first_record,
                             hipStream_t st, const uint32_t *d_labels, const uint64_t *d_label_off) {
    const int64_t n_chunks = (N + CHUNK - 1) / CHUNK;
    const int64_t rows_cap = rows_capacity(N, R);
    // (pack.hip indexes the planes and the stream with 32 bits)
    if (pack() && rows_cap * P.S > ((int64_t)1 << 32) - 4096)
        throw CapacityError("pack: the call's rows exceed 2^32 positions");
    if (pair() && rows_cap * P.S > ((int64_t)1 << 32) - 4096)  // (pair.hip: a flat 32-bit work index)
        throw CapacityError("pair: the call's rows exceed 2^32 positions");
    ranges.ensure((size_t)std::max<int64_t>(n_chunks, 1) * 3);
    // a chunk's list: STAGE u16 (WordPiece), STAGE / UNI_STAGE u32 entries (BPE / Unigram)
    const bool wp = dt.kind != TOK_BYTE_BPE && dt.kind != TOK_UNIGRAM;
    tokc.ensure((size_t)std::max<int64_t>(n_chunks, 1) * (dt.kind == TOK_UNIGRAM ? UNI_STAGE : wp ? STAGE / 2 : STAGE));
    chunk_cnt.ensure((size_t)n_chunks + 1);
    chunk_off.ensure((size_t)n_chunks + 1);
    rec_local.ensure((size_t)R + 1);
    // the dense id array: ids <= text bytes for WordPiece/BPE; Unigram adds a "▁" piece per
    // word and expanding normalizations: bound by the chunk entries + the pool.  (WordPiece
    // mlm / clm / labels: only a small call needs it, below)
    const size_t tok_ids_n = dt.kind == TOK_UNIGRAM ? (size_t)2 * N + 1024 * 1024 + 1 : (size_t)N + 1;
    if (!wp || span()) tok_ids.ensure(tok_ids_n);
    rec_tok.ensure((size_t)R + 1);
    rec_cnt.ensure((size_t)R + 1);
    rec_rows.ensure((size_t)R + 1);
    row_off.ensure((size_t)R + 1);
    scan_tmp.ensure((size_t)std::max({scan_tmp_words(n_chunks), scan_tmp_words(R), records_tile_words(R)}) + 1);
    const size_t plane = (size_t)std::max<int64_t>(rows_cap, 1) * P.S;
    o_ids.ensure(plane);
    o_am.ensure(plane);
    if (plane4()) o_tt.ensure(plane);
    if (multi()) {
        o_f32.ensure((size_t)std::max<int64_t>(rows_cap, 1) * P.label_width);
        lab_err.ensure(1);
    } else {
        o_lab.ensure((size_t)std::max<int64_t>(rows_cap, 1) * P.label_width);
        if (single()) lab_err.ensure(1);
    }
    row_rec.ensure((size_t)std::max<int64_t>(rows_cap, 1));
    const bool rm1 = P.task == SDL_TASK_MLM && P.rng_mode == 1;
    const bool policy = P.task == SDL_TASK_MLM && mpol.policy != 0;
    const int mask_w = (P.S + 31) / 32;

    RowParams p = P;
    p.first_record = first_record;
    p.mask_w = mask_w;
    p.mask_bits0 = nullptr;
    p.mask_spos = nullptr;
    p.mask_off = d_off;
    p.mask_R = R;
    p.mask_spec1 = 0;
    const bool bpe = dt.kind == TOK_BYTE_BPE;
    const bool uni = dt.kind == TOK_UNIGRAM;
    // Pipelined segments (WordPiece): the tokenize launches of the chunk
    // ranges run back to back on `st` while a second stream runs each
    // finished segment's scans, compaction, records and rows -- the
    // latency-bound tokenizer and the write-bound row assembly overlap.
    // The other tokenizers finish long items in follow-up kernels over the
    // whole call, so they run as one segment.
    SegChunks sc{};
    sc.K = 1;
    if (!bpe && !uni && !pair() && seg_target > 1 && n_chunks >= 2 * seg_min_chunks) {
        sc.K = (int)std::min<int64_t>(seg_target, n_chunks / seg_min_chunks);
        sc.K = std::min(sc.K, MAX_SEGMENTS);
    }
    for (int k = 0; k <= sc.K; ++k) sc.cb[k] = n_chunks * k / sc.K;
    seg_rb.ensure(MAX_SEGMENTS + 2);
    const bool piped = sc.K > 1;
    n_stages = piped ? 3 : kStages;
    stage_names = piped ? kPipedStageNames : kStageNames;
    auto mark = [&](int i) {
        if (profiling) HIP_TRY(hipEventRecord(ev[i], st));
    };
    // (pack = 1 takes the plain one-segment sequence up to launch_records, then pack.hip; pair = 1
    // the same without the dense copy of the ids, then pair.hip)
    const bool small = !piped && !profiling && !pack() && !pair() && n_chunks <= SMALL_CHUNKS && R <= 8192;
    // WordPiece, large calls: k_rows reads the chunk lists themselves -- no dense copy of the
    // ids (span's rows kernels and the small-call kernels read the dense array)
    const bool from_lists = wp && !small && !span();  // (pair = 1 too: k_rows_pair reads the lists)
    if (!from_lists) tok_ids.ensure(tok_ids_n);
    else if (!pair()) row_chunk.ensure((size_t)std::max<int64_t>(rows_cap, 1));  // (k_rows_pair searches the chunks itself)
    uint16_t *const lists = reinterpret_cast<uint16_t *>(tokc.p);
    mark(0);
    // (one segment: k_chunk_ranges also writes its record bounds and zeroes the label error word)
    const bool fold = sc.K == 1 && n_chunks > 0;
    // (a small push's H2D rides along: fused_h2d, set by process_host)
    HIP_TRY(launch_chunk_ranges(fused_h2d.bytes ? fused_h2d.h_off : d_off, R, N, ranges.p, st,
                                fold ? seg_rb.p : nullptr, fold && (multi() || single()) ? lab_err.p : nullptr,
                                fused_h2d.src, fused_h2d.dst, fused_h2d.bytes));
    fused_h2d = FusedH2D{};
    // rng_mode 1: a row's masks depend on (seed, record, chunk) alone, so the rows known before
    // tokenizing -- chunk 0 of every record, chunk 1 of records long enough to need one at
    // <= rand_spec_rho ids per byte -- are walked, and their mask bits made, on stream2 beside
    // the tokenizer (queued after k_chunk_ranges: launched first, their long waves held it back
    // 0.12 ms); k_rows waits for them.  Rows past the guess take the late path (correct either way).
    const bool rec0 = rm1 && !piped && !small && R > 0 && rand_rec0;
    if (rec0) {
        const int64_t F = P.n_pre + P.n_post;
        p.mask_spec1 = P.chunk && rand_spec_rho > 0 ? (int64_t)((double)(P.S - F + 1) / rand_spec_rho) : 0;
        // chunk-1 slots: the records of >= mask_spec1 bytes, at most N / mask_spec1 of them
        const int64_t ns = R + (p.mask_spec1 > 0 ? std::min<int64_t>(R, N / p.mask_spec1 + 1) : 0);
        mask_j0.ensure((size_t)ns * (size_t)P.S);
        mask_bits0.ensure((size_t)ns * (size_t)mask_w);
        spec_list.ensure((size_t)R + 1);
        spec_pos.ensure((size_t)R + 1);
        p.mask_spos = spec_pos.p;
        ensure_stream2();
        for (auto &e : rand_ev)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(rand_ev[0], st));  // (the last call's rows have read mask_bits0)
        HIP_TRY(hipStreamWaitEvent(stream2, rand_ev[0], 0));
        p.mask_bits0 = mask_bits0.p;
        HIP_TRY(launch_mask_rand_rec(p, spec_list.p, spec_pos.p, mask_j0.p, mask_bits0.p, stream2));
        HIP_TRY(hipEventRecord(rand_ev[1], stream2));
    }
    if (!fold) HIP_TRY(launch_seg_bounds(ranges.p, sc, R, seg_rb.p, st));
    if (!fold && (multi() || single())) HIP_TRY(hipMemsetAsync(lab_err.p, 0, 4, st));
    mark(1);
    RowOut out{o_ids.p, o_am.p, with_tt() ? o_tt.p : nullptr, multi() ? nullptr : o_lab.p,
               multi() ? o_f32.p : nullptr, DirectDst{}};
    // a small mlm / clm push with its host batches ready (process_host): k_rows writes them
    // and k_downstream_small the row offsets -- no k_rows_direct launch
    fused_done = small && fuse_stat && (P.task == SDL_TASK_MLM || P.task == SDL_TASK_CLM);
    if (fused_done) out.direct = fuse_dd;
    // everything after the tokenizer, for segment k, on stream s
    auto small_down = [&]() {
        SmallDown d{tokc.p, chunk_cnt.p, chunk_off.p, tok_ids.p,
                    uni ? uni_counters.p : bpe ? long_count.p : nullptr,
                    uni || bpe ? chunk_ent.p : nullptr, bpe ? long_list.p : nullptr,
                    bpe ? long_scratch.p : nullptr, uni ? uni_pool.p : nullptr,
                    uni ? (int64_t)UNI_STAGE : (int64_t)STAGE, wp ? 1 : 0, rec_local.p, rec_tok.p, rec_cnt.p,
                    rec_rows.p, row_off.p, row_rec.p, fused_done ? fuse_stat : nullptr,
                    uni ? uni_err.p : nullptr, 0, out};
        // mlm (Philox) / clm rows in the same workgroup, no k_rows launch (the BERT mask
        // policies are k_rows_policy's alone: their small calls take one launch more)
        d.rows = fused_done && !rm1 && !policy ? 1 : 0;
        return d;
    };
    auto downstream = [&](int k, hipStream_t s) {
        const SegSel sel{seg_rb.p, k, k == sc.K - 1 ? 1 : 0};
        const int64_t ca = sc.cb[k], cz = sc.cb[k + 1];
        bool rows_done = false;
        if (small) {  // one launch for the five below
            const SmallDown d = small_down();
            rows_done = d.rows != 0;
            HIP_TRY(launch_downstream_small(d, p, d_off, R, N, s));
        } else {
        if (!piped) mark(2);
        HIP_TRY(launch_exclusive_scan(chunk_cnt.p + ca, chunk_off.p + ca, cz - ca, scan_tmp.p, s,
                                      k > 0 ? chunk_off.p + ca : nullptr));
        if (!piped) mark(3);
        if (uni)
            HIP_TRY(launch_compact_tokens(tokc.p, chunk_cnt.p, chunk_off.p, n_chunks, tok_ids.p, uni_counters.p,
                                          chunk_ent.p, nullptr, nullptr, s, uni_pool.p, UNI_STAGE));
        else if (bpe)
            HIP_TRY(launch_compact_tokens(tokc.p, chunk_cnt.p, chunk_off.p, n_chunks, tok_ids.p, long_count.p,
                                          chunk_ent.p, long_list.p, long_scratch.p, s));
        else if (!from_lists)
            HIP_TRY(launch_compact_tokens(tokc.p + ca * (STAGE / 2), chunk_cnt.p + ca, chunk_off.p + ca, cz - ca,
                                          tok_ids.p, nullptr, nullptr, nullptr, nullptr, s, nullptr, STAGE, true));
        if (!piped) mark(4);
        // one segment past the one-workgroup scan: k_records leaves the row scan's tile sums
        // (scan_tmp: the chunk scan before it on the stream is done with them) and one launch
        // scans the rows and maps them, in place of reduce, sums, apply and k_row_map
        const bool scan_map = !piped && !pack() && !pair() && R > scan_small_max();
        HIP_TRY(launch_records(p, d_off, R, N, chunk_off.p, n_chunks, rec_local.p, rec_tok.p, rec_cnt.p, rec_rows.p,
                               sel, s, scan_map ? scan_tmp.p : nullptr));
        if (!piped) mark(5);
        if (pack()) {  // rec_tok / rec_cnt exist: the stream's rows instead of row scan, row map and k_rows
            mark(6);
            run_pack(R, rows_cap, s);
            return;
        }
        if (pair()) {  // a row per pair of text ranges instead of row scan, row map and k_rows
            mark(6);
            run_pair(R, rows_cap, n_chunks, d_off, first_record, s, d_labels, d_label_off);
            return;
        }
        // (segment k's rows read lists and offsets of chunks < cz only: all written by now)
        const RowChunkIn rc{row_chunk.p, rec_tok.p, rec_cnt.p, chunk_off.p, d_off, cz, P.S, P.n_pre, P.chunk};
        if (scan_map) {
            HIP_TRY(launch_scan_rows_map(rec_rows.p, R, scan_tmp.p, row_off.p, row_rec.p, s,
                                         from_lists ? &rc : nullptr));
        } else {
            if (piped) HIP_TRY(launch_scan_range(rec_rows.p, row_off.p, seg_rb.p, k, s));
            else HIP_TRY(launch_exclusive_scan(rec_rows.p, row_off.p, R, scan_tmp.p, s));
            HIP_TRY(launch_row_map(row_off.p, R, row_rec.p, sel, s, from_lists ? &rc : nullptr));
        }
        }
        const TokSrc src = from_lists ? TokSrc{nullptr, lists, chunk_off.p, cz, row_chunk.p}
                                      : TokSrc{tok_ids.p, nullptr, nullptr, 0, nullptr};
        if (!piped) mark(6);
        if (span() && snoise.counts) {  // (SDL_SPAN_TWO_PHASE has no effect: one kernel plans and writes)
            span_err.ensure(1);
            HIP_TRY(launch_rows_span_t5(p, snoise, tok_ids.p, rec_tok.p, rec_cnt.p, row_off.p, row_rec.p, sel,
                                        rows_cap, out, span_err.p, s));
        } else if (span()) {
            span_err.ensure(1);
            SpanPlan pl{};
            const bool two_phase = span_two_phase;
            if (two_phase) {
                pl.capr = P.label_width / 2 + 2;
                span_tab.ensure((size_t)std::max<int64_t>(rows_cap, 1) * (size_t)pl.capr);
                span_meta.ensure((size_t)std::max<int64_t>(rows_cap, 1));
                span_ovf.ensure((size_t)std::max<int64_t>(rows_cap, 1) + 1);
                pl.tab = span_tab.p;
                pl.meta = span_meta.p;
                pl.ovf_n = span_ovf.p;
                pl.ovf_list = span_ovf.p + 1;
            }
            HIP_TRY(launch_rows_span(p, tok_ids.p, rec_tok.p, rec_cnt.p, row_off.p, row_rec.p, sel, rows_cap, out,
                                     span_err.p, s, two_phase ? &pl : nullptr));
        } else {
            // rng_mode 1: k_rows waits for the rows walked beside the tokenizer and walks the rest
            // (and walks the rows past the guess in a second pass)
            if (rm1 && rec0) {
                HIP_TRY(hipStreamWaitEvent(s, rand_ev[1], 0));
                HIP_TRY(launch_rows(p, src, rec_tok.p, rec_cnt.p, row_off.p, row_rec.p, sel, rows_cap, out, s));
            } else if (!rows_done) {
                HIP_TRY(launch_rows(p, src, rec_tok.p, rec_cnt.p, row_off.p, row_rec.p, sel, rows_cap, out, s,
                                    nullptr, policy ? &mpol : nullptr));
            }
        }
        if (multi())
            HIP_TRY(launch_multi_labels(d_labels, d_label_off, row_rec.p, row_off.p, sel, rows_cap, P.B,
                                        P.label_width, o_f32.p, lab_err.p, s));
        else if (single())
            HIP_TRY(launch_single_labels(d_labels, d_label_off, row_rec.p, row_off.p, sel, rows_cap, P.B, o_lab.p,
                                         lab_err.p, s));
    };
    if (uni) {
        // long items: words > UNI_WMAX bytes (<= N / 25), one per chunk past
        // its window, and medium words whose normalization overflows the
        // chunk's arena: N / 8 + n_chunks bounds every realistic text (an
        // overflow is flagged in d_tokenize_errors); their ids go to the pool
        // long items: one wave each; 256 CUs x 9 resident (k_unigram_long<20>: 17 KB of LDS, 154 VGPRs)
        const int lane_blocks = 2304, huge_blocks = 8;
        uni_counters.ensure(8);
        uni_err.ensure(1);
        uni_items.ensure((size_t)(N / 8 + n_chunks + 64));
        uni_items2.ensure((size_t)(N / 64 + 64));
        uni_huge.ensure((size_t)(N / 256 + 64));
        uni_pool.ensure((size_t)N + 1024 * 1024);
        uni_scratch.ensure(unigram_scratch_bytes(lane_blocks, huge_blocks));
        chunk_ent.ensure((size_t)n_chunks + 1);
        uint32_t item_cap = (uint32_t)std::min<size_t>(uni_items.cap, 0xFFFFFFFFu);
        if (uni_item_cap) item_cap = std::min(item_cap, uni_item_cap);
        if (!stream_u) {
            HIP_TRY(hipStreamCreateWithFlags(&stream_u, hipStreamNonBlocking));
            for (auto &e : uni_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        }
        UniWork W{uni_counters.p, uni_items.p, item_cap, uni_pool.p,
                  (uint32_t)std::min<size_t>(uni_pool.cap, 0x3FFFFFFF), uni_huge.p, (uint32_t)uni_huge.cap,
                  uni_items2.p, (uint32_t)uni_items2.cap, uni_scratch.p, lane_blocks, huge_blocks, uni_err.p,
                  stream_u, uni_ev[0], uni_ev[1]};
        HIP_TRY(launch_unigram_chunks(dt, d_text, N, d_off, R, ranges.p, tokc.p, chunk_cnt.p, chunk_ent.p,
                                      rec_local.p, W, st));
        downstream(0, st);
    } else if (bpe) {
        // long pieces are > 64 bytes or run past their chunk's window (<= 1 per chunk)
        const uint32_t cap = (uint32_t)(N / 64 + n_chunks + 1);
        long_count.ensure(BPE_LONG_WORDS);  // (count, k_bpe_long cursor, overflow flag)
        long_list.ensure(cap);
        long_scratch.ensure((size_t)N + 64);
        chunk_ent.ensure((size_t)n_chunks + 1);
        HIP_TRY(launch_bpe_chunks(dt, d_text, N, d_off, R, ranges.p, tokc.p, chunk_cnt.p, chunk_ent.p,
                                  rec_local.p, long_count.p, long_list.p, cap, long_scratch.p, st));
        downstream(0, st);
    } else if (!piped) {
        HIP_TRY(launch_wordpiece_chunks(dt, dfirst, tok.cased, d_text, N, d_off, R, ranges.p, lists, chunk_cnt.p,
                                        rec_local.p, st, 0, -1));
        downstream(0, st);
    } else {
        ensure_pipe_events(sc.K);
        for (int k = 0; k < sc.K; ++k) {
            HIP_TRY(launch_wordpiece_chunks(dt, dfirst, tok.cased, d_text, N, d_off, R, ranges.p, lists, chunk_cnt.p,
                                            rec_local.p, st, sc.cb[k], sc.cb[k + 1]));
            HIP_TRY(hipEventRecord(pipe_ev[k], st));
            HIP_TRY(hipStreamWaitEvent(stream2, pipe_ev[k], 0));
            downstream(k, stream2);
        }
        mark(2);
        HIP_TRY(hipEventRecord(pipe_ev[sc.K], stream2));
        HIP_TRY(hipStreamWaitEvent(st, pipe_ev[sc.K], 0));  // the caller's stream sees every row
    }
    mark(piped ? 3 : 7);
    last_rows_cap = rows_cap;
    last_R = R;
    last_segments = sc.K;
}
void sdl_batcher::ensure_pipe_events(int K) {
    while ((int)pipe_ev.size() < K + 1) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        pipe_ev.push_back(e);
    }
    ensure_stream2();
}
// stream2 runs background work (rng_mode 1 mask walks, pipelined segments) at the lowest
// priority, so the dispatcher hands CUs to the handle's stream first
void sdl_batcher::ensure_stream2() {
    if (stream2) return;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
    HIP_TRY(hipStreamCreateWithPriority(&stream2, hipStreamNonBlocking, least));
}

// pack = 1, host path: the rows the last packed call (or flush) left in the device planes go
// to the working batch and fresh ones behind it (pack_queue.hpp); every batch they fill is
// queued, in order.  One synchronisation for the row count, one for the copy.
void sdl_batcher::queue_packed_rows() {
    pin_u32.ensure(4);
    HIP_TRY(hipMemcpyAsync(pin_u32.p, pk_meta.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t G = pin_u32.p[0];
    if (store.empty()) store.push_back(new_batch());
    const PackPlan plan = pack_queue_plan((uint32_t)store.back()->rows, (uint32_t)P.B, G);
    if (plan.segs.empty()) return;
    std::vector<HostBatch *> bs{store.back()};
    store.pop_back();
    struct Unwind {  // (a throw below: the batches not yet queued are freed)
        std::vector<HostBatch *> &v;
        ~Unwind() {
            for (HostBatch *b : v) delete b;
        }
    } unwind{bs};
    while (bs.size() < (size_t)plan.completed + 1) bs.push_back(new_batch());
    seg_pin.ensure(plan.segs.size());
    seg_dev.ensure(plan.segs.size());
    uint32_t nmax = 0;
    for (size_t i = 0; i < plan.segs.size(); ++i) {
        const PackSeg &q = plan.segs[i];
        HostBatch *b = bs[q.batch];
        seg_pin.p[i] = RowSeg{b->on_dev(b->ids), b->on_dev(b->am), b->on_dev(b->tt), b->on_dev(b->lab), q.g0, q.n,
                              q.dst, 0u};
        nmax = std::max(nmax, q.n);
    }
    HIP_TRY(hipMemcpyAsync(seg_dev.p, seg_pin.p, sizeof(RowSeg) * plan.segs.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(launch_rows_to_host(seg_dev.p, (int)plan.segs.size(), nmax, o_ids.p, o_am.p, o_tt.p, o_lab.p, P.S,
                                P.label_width, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (uint32_t k = 0; k < plan.completed; ++k) {
        bs[k]->rows = P.B;
        outbox.push_back(bs[k]);
        bs[k] = nullptr;
    }
    bs.back()->rows = (int)plan.fill;
    store.push_back(bs.back());
    bs.back() = nullptr;
}

// H2D a host arena, run the device path, bring back the rows; then play
// GenTokenizer's queue over the per-record row counts.
void sdl_batcher::process_host(const uint8_t *arena, const uint64_t *offsets, int64_t R, const uint32_t *labels,
                               const uint64_t *label_off) {
    const int64_t N = (int64_t)offsets[R];
    // pair = 1: R text ranges are E = R / 2 examples -- one label set, one row, one cadence step each
    const int64_t E = pair() ? R / 2 : R;
    // one pinned staging blob, one H2D: text | offsets | labels | label offsets
    const bool with_labels = simple() && labels && label_off;  // validated by the caller
    const uint64_t L = with_labels ? label_off[E] - label_off[0] : 0;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t x_off = up((size_t)N + 16), x_lab = up(x_off + 8 * (size_t)(R + 1)),
                 x_loff = up(x_lab + 4 * (size_t)L + 4), blob = x_loff + 8 * (size_t)(E + 1);
    pin_blob.ensure(blob + 16);  // (+16: k_chunk_ranges copies whole 16-B units)
    h2d_blob.ensure(blob + 16);
    HostClock hc;
    par_copy(pin_blob.p, arena, (size_t)N);
    hc.lap("stage");
    std::memcpy(pin_blob.p + x_off, offsets, sizeof(uint64_t) * (size_t)(R + 1));
    const uint32_t *d_labels = nullptr;
    const uint64_t *d_label_off = nullptr;
    size_t h2d_bytes = x_off + 8 * (size_t)(R + 1);
    if (with_labels) {  // Label::Multi indices / Label::Single
        std::memcpy(pin_blob.p + x_lab, labels, sizeof(uint32_t) * (size_t)L);
        uint64_t *lo = reinterpret_cast<uint64_t *>(pin_blob.p + x_loff);
        for (int64_t r = 0; r <= E; ++r) lo[r] = label_off[r] - label_off[0];
        d_labels = reinterpret_cast<const uint32_t *>(h2d_blob.p + x_lab);
        d_label_off = reinterpret_cast<const uint64_t *>(h2d_blob.p + x_loff);
        h2d_bytes = blob;
    }
    // a small push (<= 64 KiB staged): k_chunk_ranges copies the blob itself, so the stream has
    // one operation fewer before the tokenizer (the few KB cross PCIe as the kernel's loads)
    fused_h2d = FusedH2D{};
    const uint8_t *d_text = h2d_blob.p;
    const uint64_t *d_off = reinterpret_cast<const uint64_t *>(h2d_blob.p + x_off);
    if (h2d_bytes <= (64u << 10) && !profiling) {
        if (blob_dev_host != pin_blob.p) {  // (once per staging buffer)
            HIP_TRY(hipHostGetDevicePointer(&blob_dev, pin_blob.p, 0));
            blob_dev_host = pin_blob.p;
        }
        const uint8_t *dsrc = static_cast<const uint8_t *>(blob_dev);
        fused_h2d.src = dsrc;
        fused_h2d.dst = h2d_blob.p;
        fused_h2d.bytes = h2d_bytes;
        fused_h2d.h_off = reinterpret_cast<const uint64_t *>(dsrc + x_off);
    } else {
        HIP_TRY(hipMemcpyAsync(h2d_blob.p, pin_blob.p, h2d_bytes, hipMemcpyHostToDevice, stream));
    }
    // Small calls (a per-record push): the rows go straight to the back batch
    // and a pre-allocated next one in the same pass, and the row offsets and
    // error words come back through mapped memory -- one synchronisation.
    const bool direct = R <= 4096 && N <= ((int64_t)1 << 20) && !store.empty() && !profiling && !pack() && !pair();
    uint32_t cap = 0;
    const uint32_t *stat;
    DirectDst dd{};
    if (direct) {
        if (!spare) spare = new_batch();
        HostBatch *b0 = store.back(), *b1 = spare;
        cap = (uint32_t)(2 * P.B - b0->rows);
        for (int i = 0; i < 2; ++i) {
            HostBatch *b = i ? b1 : b0;
            dd.ids[i] = b->on_dev(b->ids);
            dd.am[i] = b->on_dev(b->am);
            dd.tt[i] = b->on_dev(b->tt);
            dd.lab[i] = b->on_dev(multi() ? (int32_t *)b->f32 : b->lab);
        }
        dd.base = (uint32_t)b0->rows;
        dd.cap = cap;
        dd.B = (uint32_t)P.B;
        ensure_stat((size_t)R + 3);
        fuse_dd = dd;
        fuse_stat = stat_dev;
    }
    fused_done = false;
    struct FuseReset {  // (no other entry point may see this call's destinations, also on a throw)
        uint32_t *&p;
        ~FuseReset() { p = nullptr; }
    } fuse_reset{fuse_stat};
    {
        struct Clear {  // (never left set for a later call, also on a throw)
            FusedH2D &f;
            ~Clear() { f = FusedH2D{}; }
        } clear{fused_h2d};
        run_device(d_text, N, d_off, R, first_override >= 0 ? (uint64_t)first_override : cfg.first_record + n_records,
                   stream, d_labels, d_label_off);
    }
    fuse_stat = nullptr;
    if (pack()) {  // the stream's rows fill the queue's batches; no per-record cadence
        hc.lap("enqueue");
        queue_packed_rows();
        hc.lap("h2d+kernels+d2h");
        hc.report(N, 0, pool ? pool->fresh : 0);
        n_records += (uint64_t)R;
        return;
    }
    if (direct) {
        if (!fused_done)
            HIP_TRY(launch_rows_direct(dd, row_off.p, R, o_ids.p, o_am.p, with_tt() ? o_tt.p : nullptr,
                                       multi() ? reinterpret_cast<const int32_t *>(o_f32.p) : o_lab.p, P.S,
                                       P.label_width, span() ? span_err.p : nullptr,
                                       dt.kind == TOK_UNIGRAM ? uni_err.p : nullptr, stat_dev, stream));
        hc.lap("enqueue");
        HIP_TRY(hipStreamSynchronize(stream));
        hc.lap("h2d+kernels+rows");
        stat = pin_stat.p;
    } else {
        hc.lap("enqueue");
        pin_u32.ensure((size_t)E + 3);
        HIP_TRY(hipMemcpyAsync(pin_u32.p, row_off.p, sizeof(uint32_t) * (size_t)(E + 1), hipMemcpyDeviceToHost,
                               stream));
        pin_u32.p[E + 1] = pin_u32.p[E + 2] = 0;
        if (pair_mlm()) {  // the pair labels ride the same synchronisation (row g of the call is pair g)
            pin_pair_lab.ensure((size_t)E + 1);
            HIP_TRY(hipMemcpyAsync(pin_pair_lab.p, o_pair_lab.p, sizeof(int32_t) * (size_t)E, hipMemcpyDeviceToHost,
                                   stream));
        }
        if (span()) HIP_TRY(hipMemcpyAsync(pin_u32.p + E + 1, span_err.p, 4, hipMemcpyDeviceToHost, stream));
        if (dt.kind == TOK_UNIGRAM)
            HIP_TRY(hipMemcpyAsync(pin_u32.p + E + 2, uni_err.p, 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        hc.lap("h2d+kernels");
        stat = pin_u32.p;
    }
    // where the reference panics (t5_data.rs:205-216: a label past S/4 or a
    // 101st sentinel) the host path fails the call before any batch is queued
    if (stat[E + 1])
        throw ArgError("span: " + std::to_string(stat[E + 1]) +
                       " label/sentinel writes out of range (the reference panics)");
    if (stat[E + 2])
        throw CapacityError("t5 tokenizer capacity exceeded (flags " + std::to_string(stat[E + 2]) + ")");
    // GenTokenizer::create_sync_batch per record (gen_batcher.rs:69-94):
    // rows fill the back batch (handle_internal_batch per chunk), at most
    // one finished batch is emitted per record.  Each run of rows landing
    // contiguously in one batch and not written by the direct pass is one
    // segment, copied D2H below.
    struct Seg {
        HostBatch *b;
        uint32_t dst, g0, n;
    };
    std::vector<Seg> segs;
    for (int64_t r = 0; r < E; ++r) {
        const uint32_t g0 = stat[r], g1 = stat[r + 1];
        if (g1 > g0 && store.empty())  // store.back_mut().unwrap() (gen_batcher.rs:45) panics
            throw ArgError("a record after get_working_batch emptied the batch store (the reference panics)");
        for (uint32_t g = g0; g < g1; ++g) {
            HostBatch *b = store.back();
            if (g >= cap) {
                if (!segs.empty() && segs.back().b == b && segs.back().g0 + segs.back().n == g) ++segs.back().n;
                else segs.push_back(Seg{b, (uint32_t)b->rows, g, 1u});
            }
            if (!b->pair_lab.empty()) b->pair_lab[(size_t)b->rows] = pin_pair_lab.p[g];
            b->rows++;
            if (b->rows == P.B) {
                store.push_back(spare ? spare : new_batch());
                spare = nullptr;
            }
        }
        if (!store.empty() && store.front()->rows == P.B) {  // at most one batch per call
            outbox.push_back(store.front());
            store.pop_front();
        }
    }
    hc.lap("cadence");
    if (!segs.empty()) {
        seg_pin.ensure(segs.size());
        uint32_t nmax = 0;
        for (size_t i = 0; i < segs.size(); ++i) {
            const Seg &q = segs[i];
            HostBatch *b = q.b;
            seg_pin.p[i] = RowSeg{b->on_dev(b->ids), b->on_dev(b->am), b->on_dev(b->tt),
                                  b->on_dev(multi() ? (int32_t *)b->f32 : b->lab), q.g0, q.n, q.dst, 0u};
            nmax = std::max(nmax, q.n);
        }
        seg_dev.ensure(segs.size());
        HIP_TRY(hipMemcpyAsync(seg_dev.p, seg_pin.p, sizeof(RowSeg) * segs.size(), hipMemcpyHostToDevice, stream));
        HIP_TRY(launch_rows_to_host(seg_dev.p, (int)segs.size(), nmax, o_ids.p, o_am.p,
                                    with_tt() ? o_tt.p : nullptr,
                                    multi() ? reinterpret_cast<const int32_t *>(o_f32.p) : o_lab.p, P.S,
                                    P.label_width, stream));
    }
    hc.lap("d2h enqueue");
    if (!segs.empty()) HIP_TRY(hipStreamSynchronize(stream));
    hc.lap("d2h");
    hc.report(N, segs.size(), pool ? pool->fresh : 0);
    n_records += (uint64_t)E;
}

namespace {

void fill_batch(const sdl_batcher *h, HostBatch *b, sdl_batch *out) {
    std::memset(out, 0, sizeof(*out));
    out->rows = b->rows;
    out->batch_size = b->B;
    out->sequence_length = b->S;
    out->label_width = b->LW;
    b->init_tail();
    out->input_ids = b->ids;
    out->attention_mask = b->am;
    out->token_type_ids = b->tt_is_pos ? nullptr : b->tt;  // (position_ids: sdl_batch_position_ids)
    out->labels = b->lab;
    out->labels_f32 = b->f32;
    out->owner_ = b;
    (void)h;
}

// Span draws (RNG contract): v = trunc_sat(avg - z), z ~ N(0,1),
// by CDF inversion on a 32-bit uniform -- thr[j] = floor(2^32 P(v <= kmin + j)),
// P(v <= k) = erfc((avg - k - 1) / sqrt 2) / 2; `lo` folds smaller values in
// (size: max(.., 1)).  oracle/orc_batcher.c:orc_span_table computes the same.
void span_table(double avg, int lo, int32_t *kmin, int32_t *n, uint32_t *thr) {
    double k0 = std::floor(avg - 10.0);
    if (k0 < lo) k0 = lo;
    if (k0 > 1e9) k0 = 1e9;
    *kmin = (int32_t)k0;
    int m = 0;
    for (int j = 0; j < 32; ++j) {
        const double cdf = 0.5 * std::erfc((avg - (k0 + j) - 1.0) / std::sqrt(2.0));
        const double t = std::floor(cdf * 4294967296.0);
        if (t >= 4294967296.0) break;
        thr[m++] = (uint32_t)t;
    }
    *n = m;
    for (int j = m; j < 32; ++j) thr[j] = 0xFFFFFFFFu;
}

// rand_distr 0.4.3's ziggurat tables for StandardNormal (ZIG_NORM_X /
// ZIG_NORM_F) as its ziggurat_tables.py writes them: 256 layers with
// R = 3.6541528853610088, V = 0.00492867323399, x[i] = f^-1(V / x[i-1] +
// f(x[i-1])), f(x) = exp(-x^2 / 2), each value printed with %.18f and read
// back as the Rust literal.  (oracle/orc_batcher.c zig_tables is the checker's
// restatement; tests/test_rand_mode.py pins the printed head of both.)
void zig_norm_tables(double *X, double *F) {
    const double R = 3.6541528853610088, V = 0.00492867323399;
    auto f = [](double x) { return std::exp(-x * x / 2.0); };
    double x[257];
    x[0] = V / f(R);
    x[1] = R;
    for (int i = 2; i < 256; ++i) x[i] = std::sqrt(-2.0 * std::log(V / x[i - 1] + f(x[i - 1])));
    x[256] = 0.0;
    char buf[64];
    for (int i = 0; i < 257; ++i) {
        std::snprintf(buf, sizeof buf, "%.18f", x[i]);
        X[i] = std::strtod(buf, nullptr);
        std::snprintf(buf, sizeof buf, "%.18f", f(x[i]));
        F[i] = std::strtod(buf, nullptr);
    }
}

std::string default_data_dir() {
    Dl_info info;
    if (dladdr((void *)&default_data_dir, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        size_t s = p.rfind('/');
        return (s == std::string::npos ? std::string(".") : p.substr(0, s)) + "/data";
    }
    return "data";
}

// sdl_batcher_create's refusals of a configuration, made before a device is looked for
int check_config(const sdl_config *cfg) {
    if (cfg->task != SDL_TASK_MLM && cfg->task != SDL_TASK_CLM && cfg->task != SDL_TASK_MULTI_LABEL &&
        cfg->task != SDL_TASK_SPAN && cfg->task != SDL_TASK_SINGLE_CLASS)
        return fail(SDL_ERR_UNSUPPORTED, "unknown task");
    // (sentence pairs first: a task or tokenizer they are not built for is named as that)
    if (cfg->pair < SDL_PAIR_NONE || cfg->pair > SDL_PAIR_MLM_SOP)
        return fail(SDL_ERR_ARG, "pair must be 0 (one text per record), 1 (sentence pairs) or 2..4 (mlm sentence pairs); "
                                 "other values are reserved");
    if (cfg->pair >= SDL_PAIR_MLM) {
        if (cfg->task != SDL_TASK_MLM)
            return fail(SDL_ERR_ARG, "pair = 2..4 (mlm sentence pairs, NSP / SOP draws) apply to the MLM task only");
        if (cfg->mask_policy == SDL_MASK_REFERENCE)
            return fail(SDL_ERR_UNSUPPORTED,
                        "pair = 2..4 with mask_policy 0: the reference's rule masks [CLS] / [SEP] and defines nothing "
                        "for pairs; use mask_policy 1 or 2");
        if (cfg->rng_mode == 1)
            return fail(SDL_ERR_UNSUPPORTED, "pair = 2..4 need rng_mode 0: the draw and the masks are on the Philox contract");
        if (cfg->sequence_length < 3)
            return fail(SDL_ERR_ARG, "pair = 2..4 need sequence_length >= 3: [CLS] A [SEP] B [SEP]");
        if (cfg->sequence_length > 2048)
            return fail(SDL_ERR_ARG, "pair = 2..4 need sequence_length <= 2048 (the masking kernels' limit)");
    }
    if (cfg->pair == SDL_PAIR_ROWS) {
        if (cfg->task != SDL_TASK_SINGLE_CLASS && cfg->task != SDL_TASK_MULTI_LABEL)
            return fail(SDL_ERR_UNSUPPORTED,
                        "pair = 1 with task mlm, clm or span: sentence pairs are built for the single-class and "
                        "multi-label tasks only");
        if (cfg->sequence_length < 3)
            return fail(SDL_ERR_ARG, "pair = 1 needs sequence_length >= 3: [CLS] A [SEP] B [SEP]");
    }
    if (cfg->task == SDL_TASK_SPAN && (cfg->sequence_length < 4 || !(cfg->avg_span_gap == cfg->avg_span_gap) ||
                                       !(cfg->avg_span_size == cfg->avg_span_size)))
        return fail(SDL_ERR_ARG, "span needs sequence_length >= 4 and finite avg_span_gap / avg_span_size");
    if (cfg->task == SDL_TASK_MULTI_LABEL && (cfg->number_labels <= 0 || cfg->number_labels > 4096))
        return fail(SDL_ERR_ARG, "number_labels must be in [1, 4096]");
    if (cfg->batch_size <= 0 || cfg->sequence_length <= 0 || cfg->sequence_length > 2048)
        return fail(SDL_ERR_ARG, "batch_size must be > 0 and 0 < sequence_length <= 2048");
    if (cfg->task == SDL_TASK_MLM && (cfg->mask_length < 0 || cfg->mask_length > cfg->sequence_length))
        return fail(SDL_ERR_ARG, "mask_length must be in [0, sequence_length]");
    if (cfg->rng_mode != 0 && cfg->rng_mode != 1) return fail(SDL_ERR_ARG, "rng_mode must be 0 or 1");
    if (cfg->task == SDL_TASK_MLM && cfg->rng_mode == 1 && cfg->sequence_length > RAND_MAX_S)
        return fail(SDL_ERR_UNSUPPORTED, "rng_mode 1 supports sequence_length <= 2048");
    if (cfg->mask_policy < SDL_MASK_REFERENCE || cfg->mask_policy > SDL_MASK_BERT_WHOLE_WORD)
        return fail(SDL_ERR_ARG, "mask_policy must be 0 (reference), 1 (BERT) or 2 (BERT whole word)");
    if (cfg->mask_policy != SDL_MASK_REFERENCE) {
        if (cfg->task != SDL_TASK_MLM) return fail(SDL_ERR_ARG, "mask_policy 1 / 2 apply to the MLM task only");
        if (cfg->mask_per_mille < 1 || cfg->mask_per_mille > 1000)
            return fail(SDL_ERR_ARG, "mask_per_mille must be in [1, 1000] under mask_policy 1 / 2");
        if (cfg->rng_mode == 1)
            return fail(SDL_ERR_UNSUPPORTED,
                        "mask_policy 1 / 2 need rng_mode 0: the reference's own draws define no such policy");
    }
    if (cfg->pack != 0 && cfg->pack != 1) return fail(SDL_ERR_ARG, "pack must be 0 (off) or 1 (packed rows)");
    if (cfg->pack == 1 && cfg->task != SDL_TASK_CLM) return fail(SDL_ERR_ARG, "pack = 1 applies to the CLM task only");
    if (cfg->span_policy < SDL_SPAN_REFERENCE || cfg->span_policy > SDL_SPAN_T5)
        return fail(SDL_ERR_ARG, "span_policy must be 0 (reference) or 1 (T5)");
    if (cfg->span_policy == SDL_SPAN_T5) {
        if (cfg->task != SDL_TASK_SPAN) return fail(SDL_ERR_ARG, "span_policy 1 applies to the span task only");
        if (cfg->span_noise_per_mille < 1 || cfg->span_noise_per_mille > 500)
            return fail(SDL_ERR_ARG, "span_noise_per_mille must be in [1, 500] under span_policy 1");
        if (!std::isfinite(cfg->avg_span_size) || cfg->avg_span_size < 1.0)
            return fail(SDL_ERR_ARG, "span_policy 1 reads avg_span_size as the mean noise span length: finite and >= 1.0");
        if (cfg->rng_mode == 1)
            return fail(SDL_ERR_UNSUPPORTED,
                        "span_policy 1 needs rng_mode 0: the reference's own draws define no such policy");
        // the full row is the worst case: t, m and t + m never decrease with n
        int t = 0, m = 0;
        const int S = cfg->sequence_length, LW = S / 4;
        span_noise_counts(S, cfg->span_noise_per_mille, cfg->avg_span_size, &t, &m);
        if (t + m + 1 > LW || m + 1 > SPAN_MAX_SENTINELS)
            return fail(SDL_ERR_ARG,
                        "span_policy 1: a full row of " + std::to_string(S) + " ids has " + std::to_string(t) +
                            " noise ids in " + std::to_string(m) + " spans and needs " + std::to_string(t + m + 1) +
                            " labels and " + std::to_string(m + 1) + " sentinels; the row holds " +
                            std::to_string(LW) + " labels (S/4) and the vocabulary " +
                            std::to_string(SPAN_MAX_SENTINELS) + " sentinels: lower span_noise_per_mille or raise avg_span_size");
    }
    return SDL_OK;
}

// the tokenizer tables to the device, DevTok and DevFirst filled with their addresses
void upload_tables(sdl_batcher *h) {
    auto &t = h->tok;
    DevTok &d = h->dt;
    d.ubmp = reinterpret_cast<const uint2 *>(h->d_ubmp.upload(t.ubmp));
    h->d_ascii_id.ensure(128);
    if (t.ascii_id.size() == 128) h->d_ascii_id.upload(t.ascii_id);
    d.upage = h->d_upage.upload(t.upage);
    d.uentry = h->d_uentry.upload(t.uentry);
    d.upool = h->d_upool.upload(t.upool);
    if (t.kind == TOK_UNIGRAM) {
        // the device copy of the pieces table: a piece whose f64 score is one ulp
        // off its f32 has bit 15 of its id set, and the f32 in word 3 negated when
        // the ulp is towards zero (tokenize_unigram.hip uni_score64)
        std::vector<VSlot> ds(t.slots);
        for (VSlot &v : ds) {
            const uint32_t cont = v.key >> 8;
            if (v.id < 0 || (cont != UC_PIECE && cont != UC_META)) continue;
            const int adj = t.uscore_adj[(size_t)v.id];
            if (adj == 0) continue;
            const float f = t.uscore32[(size_t)v.id];
            // (0x7FFF | 0x8000 is the chunk kernel's "no piece" word: tokenize_unigram.hip NO_PIECE)
            if (v.id >= 0x7FFF || !(f < 0.0f))
                throw std::runtime_error("Unigram: a score off its f32 needs id < 32767 and a negative score");
            v.id |= 0x8000;
            if (adj < 0) {
                const float g = -f;
                std::memcpy(&v.hash, &g, 4);
            }
        }
        h->d_slots.upload(ds);
    } else {
        h->d_slots.upload(t.slots);
    }
    d.vpool = h->d_vpool.upload(t.vpool);
    d.kind = t.kind;
    if (t.kind == TOK_BYTE_BPE) {
        d.gpage = h->d_gpage.upload(t.gpage);
        d.gblock = h->d_gblock.upload(t.gblock);
        d.mslots = h->d_mslots.upload(t.mslots);
        d.byte_id = h->d_byte_id.upload(t.byte_id.data(), 256);
        d.mslot_mask = t.mslot_mask;
    }
    if (t.kind == TOK_UNIGRAM) {
        d.uscore = h->d_uscore.upload(t.uscore);
        d.wres = h->d_wres.upload(t.wres);
        d.cpage = h->d_cpage.upload(t.cpage);
        h->d_cent.ensure(t.cent.size() / 2);  // (x, y) pairs
        HIP_TRY(hipMemcpy(h->d_cent.p, t.cent.data(), t.cent.size() * 4, hipMemcpyHostToDevice));
        d.cent = h->d_cent.p;
        d.uscore32 = h->d_uscore32.upload(t.uscore32);
        d.trie = h->d_trie.upload(t.trie);
        d.tnorm = h->d_tnorm.upload(t.tnorm);
        h->d_extra.upload(t.extra_ids.data(), 100);
        d.wslots = h->d_wslots.upload(t.wslots);
        d.wslot_mask = t.wslot_mask;
        d.upfx = h->d_upfx.upload(t.upfx);
        {  // the BMP entries flattened: one dependent load per char instead of two
            std::vector<uint32_t> flat(2 * 0x10000);
            for (uint32_t cp = 0; cp < 0x10000; ++cp) {
                const size_t at = 2 * ((size_t)t.cpage[cp >> 8] * 256 + (cp & 255));
                flat[2 * cp] = t.cent[at];
                flat[2 * cp + 1] = t.cent[at + 1];
            }
            // the kernels compute White_Space and the ASCII property bytes
            // (uni_white_space / uni_ascii_props): the tables must agree
            for (uint32_t cp = 0; cp < 0x110000; ++cp) {
                const uint32_t x = t.cent[2 * ((size_t)t.cpage[cp >> 8] * 256 + (cp & 255))] & 0xFFu;
                if (((x & GP_WS) != 0) != uni_white_space(cp) || (cp < 0x80 && x != uni_ascii_props(cp)))
                    throw std::runtime_error("t5 grapheme table: White_Space / ASCII properties differ from "
                                             "the kernels' built-in ones at U+" + std::to_string(cp));
            }
            h->d_cbmp.ensure(0x10000);
            HIP_TRY(hipMemcpy(h->d_cbmp.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
            d.cbmp = h->d_cbmp.p;
        }
        d.trie_units = (uint32_t)t.trie.size();
        d.tnorm_len = (uint32_t)t.tnorm.size();
        d.unk_score = t.unk_score;
        d.maxlen_meta = t.maxlen_cont;
        d.maxlen_word = t.max_word;
        d.maxlen_piece = t.maxlen_piece;
    }
    if (h->cfg.task == SDL_TASK_SPAN && t.kind != TOK_UNIGRAM)
        throw std::runtime_error("task span needs the t5 (Unigram) tokenizer: TokenizerInfo.extra (tokenizer_wrapper.rs:77-80)");
    d.slots = h->d_slots.p;
    d.slot_mask = t.slot_mask;
    d.unk_id = t.unk_id;
    d.maxlen_first = t.maxlen_first;
    d.maxlen_cont = t.maxlen_cont;
    {
        std::vector<uint8_t> all(2 * LW_MAX, 0);
        for (int c = 0; c < 2; ++c) {
            std::vector<uint8_t> lens = t.wp_lens[c];
            std::sort(lens.begin(), lens.end());
            d.wp_nlens[c] = (int32_t)lens.size();
            std::copy(lens.begin(), lens.end(), all.begin() + c * LW_MAX);
        }
        d.wp_lens = h->d_wp_lens.upload(all);
    }
    d.wp_long_pieces = t.wp_long_pieces ? 1 : 0;
    if (t.kind == TOK_WORDPIECE) {
        h->dfirst = DevFirst{reinterpret_cast<const uint4 *>(h->d_first_slots.upload(t.first_slots)), t.first_mask,
                             t.first_seed, t.first_maxlen};
    }
    d.ascii_id = h->d_ascii_id.p;
    d.n_special = (int)t.added.size();
    d.max_special_len = t.max_special_len;
    d.opener = t.opener;
    for (size_t i = 0; i < t.added.size() && t.kind != TOK_UNIGRAM; ++i) {
        d.special_id[i] = t.added[i].second;
        d.special_len[i] = (uint8_t)t.added[i].first.size();
        std::memcpy(d.special_bytes[i], t.added[i].first.data(), t.added[i].first.size());
    }
}

// RowParams, MaskPolicy and SpanNoise from the configuration and the tokenizer, their small tables uploaded
void fill_row_params(sdl_batcher *h) {
    const sdl_config *cfg = &h->cfg;
    auto &t = h->tok;
    RowParams &P = h->P;
    P.task = cfg->task;
    P.B = cfg->batch_size;
    P.S = cfg->sequence_length;
    P.chunk = cfg->chunk;
    P.min_ids = cfg->min_ids;
    P.mask_length = cfg->mask_length;
    P.mask_id = cfg->mask_id;
    P.label_width = cfg->task == SDL_TASK_MULTI_LABEL    ? cfg->number_labels
                    : cfg->task == SDL_TASK_SINGLE_CLASS ? 1
                    : cfg->task == SDL_TASK_SPAN          ? cfg->sequence_length / 4  // t5_data.rs:44
                                                          : cfg->sequence_length;
    if (cfg->task == SDL_TASK_SPAN) {
        span_table(cfg->avg_span_gap, 0, &P.gap_kmin, &P.gap_n, P.gap_thr);
        span_table(cfg->avg_span_size, 1, &P.size_kmin, &P.size_n, P.size_thr);
        P.extra_ids = h->d_extra.p;
        P.avg_span_gap = cfg->avg_span_gap;
        P.avg_span_size = cfg->avg_span_size;
        if (cfg->rng_mode == 1) {  // random_data_gap / random_data_size on the row's StdRng
            std::vector<double> zt(2 * 257);
            zig_norm_tables(zt.data(), zt.data() + 257);
            P.zig_x = h->d_zig.upload(zt);
            P.zig_f = h->d_zig.p + 257;
        }
        if (cfg->span_policy == SDL_SPAN_T5) {  // the counts' one double step stays on the host
            std::vector<uint32_t> tab((size_t)cfg->sequence_length + 1);
            span_noise_table(cfg->sequence_length, cfg->span_noise_per_mille, cfg->avg_span_size, tab.data());
            h->snoise.counts = h->d_span_counts.upload(tab);
        }
    }
    if (cfg->task == SDL_TASK_MULTI_LABEL || cfg->task == SDL_TASK_SINGLE_CLASS) {  // SimpleBatcher: one row per record, no filter
        P.chunk = 0;
        P.min_ids = 0;
    }
    if (cfg->pair >= SDL_PAIR_MLM) {  // mlm sentence pairs: one row per pair, `chunk` and `min_ids` ignored
        P.chunk = 0;
        P.min_ids = 0;
    }
    P.seed = cfg->seed;
    P.rng_mode = cfg->rng_mode;
    h->mpol = MaskPolicy{cfg->mask_policy, cfg->mask_per_mille, (uint32_t)t.pieces.size(), 0u, nullptr};
    if (cfg->mask_policy == SDL_MASK_BERT_WHOLE_WORD) {
        h->mpol.cont_bits = h->d_cont_bits.upload(t.cont_bits);
    }
    if (t.kind == TOK_UNIGRAM) {
        // encode_mask framing for T5 (tokenizer_wrapper.rs:125-131): [eos] + template($A </s>) + [eos]
        P.n_pre = 1;
        P.pre[0] = t.eos_id;
        P.n_post = 2;
        P.post[0] = t.tpl_eos;
        P.post[1] = t.eos_id;
    } else if (t.kind == TOK_BYTE_BPE) {
        // encode_mask framing for Gpt (tokenizer_wrapper.rs:118-124): [eos] + ids + [eos]
        P.n_pre = 1;
        P.pre[0] = t.eos_id;
        P.n_post = 1;
        P.post[0] = t.eos_id;
    } else {
        // encode_mask framing (tokenizer_wrapper.rs:107-116): [CLS] + template([CLS] $A [SEP]) + [SEP] [SEP]
        P.n_pre = 2;
        P.pre[0] = t.cls_id;
        P.pre[1] = t.tpl_cls;
        P.n_post = 3;
        P.post[0] = t.tpl_sep;
        P.post[1] = t.sep_id;
        P.post[2] = t.sep_id;
    }
}

// BertData::put_data panics on an index >= number_labels (bert_data.rs:70-72)
int check_labels(const sdl_batcher *h, const uint32_t *labels, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (labels[i] >= (uint32_t)h->P.label_width)
            return fail(SDL_ERR_ARG, "label index " + std::to_string(labels[i]) + " >= number_labels");
    return SDL_OK;
}

// sdl_batcher_push_many / _push_many_pairs behind their handle checks: n_records text ranges are
// n_examples examples (the same, or half as many), each with one set of labels
int push_many_checked(sdl_batcher *h, const uint8_t *arena, const uint64_t *offsets, size_t n_records,
                             size_t n_examples, const uint32_t *labels, const uint64_t *label_offsets,
                             size_t *n_emitted) {
    if (h->multi() && label_offsets) {
        if (!labels && label_offsets[n_examples] != label_offsets[0]) return fail(SDL_ERR_ARG, "null labels");
        for (size_t r = 0; r < n_examples; ++r)
            if (label_offsets[r + 1] < label_offsets[r]) return fail(SDL_ERR_ARG, "label_offsets must be non-decreasing");
        if (int rc = check_labels(h, labels + label_offsets[0], label_offsets[n_examples] - label_offsets[0])) return rc;
    }
    if (h->single()) {
        if (!label_offsets || !labels) return fail(SDL_ERR_ARG, "single-class records need their labels");
        for (size_t r = 0; r < n_examples; ++r)
            if (label_offsets[r + 1] != label_offsets[r] + 1)
                return fail(SDL_ERR_ARG, "single-class records carry exactly one label");
    }
    if (offsets[0] != 0) return fail(SDL_ERR_ARG, "offsets[0] must be 0");
    for (size_t r = 0; r < n_records; ++r)
        if (offsets[r + 1] < offsets[r]) return fail(SDL_ERR_ARG, "offsets must be non-decreasing");
    if (offsets[n_records] >= (1ull << 32)) return fail(SDL_ERR_CAPACITY, "arena must be < 4 GiB per call");
    return guarded(SDL_ERR_CAPACITY, SDL_ERR_ARG, [&]() -> int {
        const size_t before = h->outbox.size();
        if (n_records)
            h->process_host(arena, offsets, (int64_t)n_records, labels ? labels + (label_offsets ? label_offsets[0] : 0) : nullptr,
                            label_offsets);
        if (n_emitted) *n_emitted = h->outbox.size() - before;
        return SDL_OK;
    });
}

// sdl_process_device_labels / _pairs behind their handle checks: n_records text ranges give
// n_examples examples (the same, or half as many); d_rows is row_off[n_examples]
int process_device_checked(sdl_batcher *h, const uint8_t *d_text, uint64_t text_len, const uint64_t *d_offsets,
                                  uint64_t n_records, uint64_t n_examples, const uint32_t *d_labels,
                                  const uint64_t *d_label_offsets, uint64_t first_record, void *stream,
                                  sdl_device_rows *out) {
    if ((d_labels == nullptr) != (d_label_offsets == nullptr)) return fail(SDL_ERR_ARG, "labels need label offsets");
    if (text_len >= (1ull << 32)) return fail(SDL_ERR_CAPACITY, "arena must be < 4 GiB per call");
    if (((uintptr_t)d_text & 15u) != 0) return fail(SDL_ERR_ARG, "d_text must be 16-byte aligned");
    return guarded(SDL_ERR_ARG, SDL_ERR_ARG, [&]() -> int {
        hipStream_t st = stream ? (hipStream_t)stream : h->stream;
        h->run_device(d_text, (int64_t)text_len, d_offsets, (int64_t)n_records, first_record, st, d_labels,
                      d_label_offsets);
        std::memset(out, 0, sizeof(*out));
        out->input_ids = h->o_ids.p;
        out->attention_mask = h->o_am.p;
        out->token_type_ids = h->with_tt() ? h->o_tt.p : nullptr;
        out->labels = h->multi() ? nullptr : h->o_lab.p;
        out->labels_f32 = h->multi() ? h->o_f32.p : nullptr;
        out->d_label_errors = h->simple() ? h->lab_err.p : h->span() ? h->span_err.p : nullptr;
        out->d_tokenize_errors = h->dt.kind == TOK_UNIGRAM    ? h->uni_err.p
                                 : h->dt.kind == TOK_BYTE_BPE && h->long_count.p
                                     ? h->long_count.p + BPE_LONG_ERR  // k_bpe_long's list overflow
                                     : nullptr;
        out->d_rows = h->pack() ? h->pk_meta.p : h->row_off.p + n_examples;
        out->d_record_rows = h->rec_rows.p;
        out->d_tokens = h->chunk_off.p + (text_len + CHUNK - 1) / CHUNK;
        out->rows_capacity = (uint64_t)h->last_rows_cap;
        out->label_width = h->P.label_width;
        return SDL_OK;
    });
}

}  // namespace

extern "C" {

int sdl_abi_version(void) { return SDL_ABI_VERSION; }
const char *sdl_last_error(void) { return g_err.c_str(); }

void sdl_config_default(sdl_config *c, int32_t task) {
    std::memset(c, 0, sizeof(*c));
    c->task = task;
    c->batch_size = 4096;  // masking_cases.rs:43
    c->sequence_length = 128;
    const bool simple = task == SDL_TASK_MULTI_LABEL || task == SDL_TASK_SINGLE_CLASS;
    c->chunk = simple ? 0 : 1;
    c->min_ids = simple ? 0 : 64;
    if (task == SDL_TASK_SINGLE_CLASS) c->batch_size = 2048;  // single_cases.rs (Imdb)
    c->mask_length = (int32_t)((float)c->sequence_length * 0.15f);  // masking_cases.rs:34-36
    c->mask_id = 103;
    c->number_labels = 9;
    c->avg_span_gap = 16.0;
    c->avg_span_size = 2.0;
    c->seed = 0;
    c->first_record = 0;
    c->device = 0;
    c->mask_policy = SDL_MASK_REFERENCE;
    c->mask_per_mille = 150;  // BERT's masked_lm_prob, used by policies 1 and 2 only
}

int sdl_batcher_create(const sdl_config *cfg, const char *tokenizer_path, const char *data_dir, sdl_batcher **out) {
    if (!cfg || !tokenizer_path || !out) return fail(SDL_ERR_ARG, "null argument");
    *out = nullptr;
    if (int rc = check_config(cfg)) return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(SDL_ERR_NODEV, "no HIP device visible: the Batcher runs only on the GPU (no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(SDL_ERR_ARG, "device ordinal out of range");
    std::unique_ptr<sdl_batcher> h(new sdl_batcher());
    return guarded(SDL_ERR_IO, SDL_ERR_IO, [&]() -> int {
        h->cfg = *cfg;
        h->device = cfg->device;
        load_tokenizer(tokenizer_path, data_dir ? std::string(data_dir) : default_data_dir(), h->tok);
        // (mlm sentence pairs first, so that the refusal names them also under mask_policy 2)
        if (cfg->pair >= SDL_PAIR_MLM && (h->tok.kind != TOK_WORDPIECE || h->tok.cls_id < 0 || h->tok.sep_id < 0))
            return fail(SDL_ERR_UNSUPPORTED,
                        "pair = 2..4 with a byte-level BPE or Unigram tokenizer: mlm sentence pairs need a WordPiece "
                        "tokenizer with [CLS] and [SEP] ids");
        if (cfg->mask_policy == SDL_MASK_BERT_WHOLE_WORD && h->tok.kind != TOK_WORDPIECE)
            return fail(SDL_ERR_UNSUPPORTED,
                        "mask_policy 2 (SDL_MASK_BERT_WHOLE_WORD) needs a WordPiece tokenizer: whole words are "
                        "not defined for byte-level BPE or Unigram pieces");
        if (cfg->pack == 1 && (h->tok.kind != TOK_BYTE_BPE || h->tok.eos_id < 0))
            return fail(SDL_ERR_UNSUPPORTED,
                        "pack = 1 needs a byte-level BPE tokenizer with an <|endoftext|> id: packed rows are "
                        "not built for WordPiece or Unigram tokenizers");
        if (cfg->pair == 1 && (h->tok.kind != TOK_WORDPIECE || h->tok.cls_id < 0 || h->tok.sep_id < 0))
            return fail(SDL_ERR_UNSUPPORTED,
                        "pair = 1 with a byte-level BPE or Unigram tokenizer: sentence pairs need a WordPiece "
                        "tokenizer with [CLS] and [SEP] ids");
        HIP_TRY(hipSetDevice(h->device));
        {  // the handle's stream at the highest priority (stream2's background work yields to it)
            int least = 0, greatest = 0;
            if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
            HIP_TRY(hipStreamCreateWithPriority(&h->stream, hipStreamNonBlocking, greatest));
        }
        for (auto &e : h->ev) HIP_TRY(hipEventCreate(&e));
        upload_tables(h.get());
        fill_row_params(h.get());
        if (h->pack()) {  // an empty carry in both halves
            h->pk_carry.ensure(4 * (size_t)h->P.S);
            h->pk_meta.ensure(4);
            HIP_TRY(hipMemsetAsync(h->pk_meta.p, 0, 4 * sizeof(uint32_t), h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));  // (the first call may come on a caller's stream)
        }
        h->store.push_back(h->new_batch());  // GenTokenizer::new: first DataSet
        *out = h.release();
        return SDL_OK;
    });
}

void sdl_batcher_destroy(sdl_batcher *h) { delete h; }

int sdl_batcher_push(sdl_batcher *h, const uint8_t *utf8, size_t len, const uint32_t *labels, size_t n_labels,
                     sdl_batch *out) {
    if (!h || (!utf8 && len) || (!labels && n_labels)) return fail(SDL_ERR_ARG, "null argument");
    if (h->pair()) return fail(SDL_ERR_STATE, "sdl_batcher_push on a handle created with pair = 1: use sdl_batcher_push_pair");
    if (h->multi()) {
        if (int rc = check_labels(h, labels, n_labels)) return rc;
    }
    if (h->single() && n_labels != 1) return fail(SDL_ERR_ARG, "single-class records carry exactly one label");
    if (len >= (1ull << 32)) return fail(SDL_ERR_CAPACITY, "record too large");
    return guarded(SDL_ERR_CAPACITY, SDL_ERR_ARG, [&]() -> int {
        uint64_t offs[2] = {0, (uint64_t)len};
        uint64_t loffs[2] = {0, (uint64_t)n_labels};
        const size_t before = h->outbox.size();
        h->process_host(utf8 ? utf8 : (const uint8_t *)"", offs, 1, labels, loffs);
        if (h->pack()) {  // push_many of one record: the front of the queue, the rest wait for sdl_batcher_next
            if (h->outbox.empty()) return 0;
            HostBatch *b = h->outbox.front();
            h->outbox.pop_front();
            if (out) fill_batch(h, b, out);
            else delete b;
            return 1;
        }
        if (h->outbox.size() > before) {
            HostBatch *b = h->outbox.back();
            h->outbox.pop_back();
            if (out) fill_batch(h, b, out);
            else delete b;
            return 1;
        }
        return 0;
    });
}

int sdl_batcher_push_many(sdl_batcher *h, const uint8_t *arena, const uint64_t *offsets, size_t n_records,
                          const uint32_t *labels, const uint64_t *label_offsets, size_t *n_emitted) {
    if (!h || !offsets || (!arena && n_records && offsets[n_records])) return fail(SDL_ERR_ARG, "null argument");
    if (h->pair())
        return fail(SDL_ERR_STATE, "sdl_batcher_push_many on a handle created with pair = 1: use sdl_batcher_push_many_pairs");
    return push_many_checked(h, arena, offsets, n_records, n_records, labels, label_offsets, n_emitted);
}

int sdl_batcher_push_many_pairs(sdl_batcher *h, const uint8_t *arena, const uint64_t *offsets, size_t n_pairs,
                                const uint32_t *labels, const uint64_t *label_offsets, size_t *n_emitted) {
    if (!h || !offsets || (!arena && n_pairs && offsets[2 * n_pairs])) return fail(SDL_ERR_ARG, "null argument");
    if (!h->pair()) return fail(SDL_ERR_STATE, "sdl_batcher_push_many_pairs needs a handle created with pair = 1");
    return push_many_checked(h, arena, offsets, 2 * n_pairs, n_pairs, labels, label_offsets, n_emitted);
}

// One example of two texts: push_many_pairs of one pair, staged back to back (the bulk path's
// launches and two synchronisations a call; a tuned one-pair push is not built).
int sdl_batcher_push_pair(sdl_batcher *h, const uint8_t *a, size_t len_a, const uint8_t *b, size_t len_b,
                          const uint32_t *labels, size_t n_labels, sdl_batch *out) {
    if (!h || (!a && len_a) || (!b && len_b) || (!labels && n_labels)) return fail(SDL_ERR_ARG, "null argument");
    if (!h->pair()) return fail(SDL_ERR_STATE, "sdl_batcher_push_pair needs a handle created with pair = 1");
    if (h->cfg.pair == SDL_PAIR_MLM_NSP)
        return fail(SDL_ERR_UNSUPPORTED,
                    "sdl_batcher_push_pair under pair = 3: a call of one pair has nobody to draw a next sentence "
                    "from; use sdl_batcher_push_many_pairs");
    if (h->multi()) {
        if (int rc = check_labels(h, labels, n_labels)) return rc;
    }
    if (h->single() && n_labels != 1) return fail(SDL_ERR_ARG, "single-class records carry exactly one label");
    if ((uint64_t)len_a + (uint64_t)len_b >= (1ull << 32)) return fail(SDL_ERR_CAPACITY, "record too large");
    return guarded(SDL_ERR_CAPACITY, SDL_ERR_ARG, [&]() -> int {
        std::vector<uint8_t> both(len_a + len_b);
        if (len_a) std::memcpy(both.data(), a, len_a);
        if (len_b) std::memcpy(both.data() + len_a, b, len_b);
        uint64_t offs[3] = {0, (uint64_t)len_a, (uint64_t)(len_a + len_b)};
        uint64_t loffs[2] = {0, (uint64_t)n_labels};
        const size_t before = h->outbox.size();
        h->process_host(both.empty() ? (const uint8_t *)"" : both.data(), offs, 2, labels, loffs);
        if (h->outbox.size() > before) {
            HostBatch *bt = h->outbox.back();
            h->outbox.pop_back();
            if (out) fill_batch(h, bt, out);
            else delete bt;
            return 1;
        }
        return 0;
    });
}

int sdl_batcher_next(sdl_batcher *h, sdl_batch *out) {
    if (!h || !out) return fail(SDL_ERR_ARG, "null argument");
    if (h->outbox.empty()) return 0;
    HostBatch *b = h->outbox.front();
    h->outbox.pop_front();
    fill_batch(h, b, out);
    return 1;
}

int sdl_batcher_flush(sdl_batcher *h, sdl_batch *out) {
    if (!h || !out) return fail(SDL_ERR_ARG, "null argument");
    if (h->pack()) {
        // the carry becomes the flush row behind the queued rows; then the front of the queue:
        // the full batches first, the partial one last, nothing once no filled row is left
        const int rc = guarded(SDL_ERR_ARG, SDL_ERR_ARG, [&]() -> int {
            h->run_pack_flush(h->stream);
            h->queue_packed_rows();
            return SDL_OK;
        });
        if (rc) return rc;
        HostBatch *b = nullptr;
        if (!h->outbox.empty()) {
            b = h->outbox.front();
            h->outbox.pop_front();
        } else if (!h->store.empty() && h->store.front()->rows > 0) {
            b = h->store.front();
            h->store.pop_front();
        }
        if (!b) return 0;
        fill_batch(h, b, out);
        return 1;
    }
    if (h->store.empty()) return 0;  // GenTokenizer::get_working_batch = store.pop_front()
    HostBatch *b = h->store.front();
    h->store.pop_front();
    // SimpleBatcher::get_working_batch swaps in a fresh DataSet (simple_batcher.rs:46-52)
    if (h->simple() && h->store.empty()) h->store.push_back(h->new_batch());
    fill_batch(h, b, out);
    return 1;
}

void sdl_batch_release(sdl_batch *b) {
    if (!b || !b->owner_) return;
    delete static_cast<HostBatch *>(b->owner_);
    std::memset(b, 0, sizeof(*b));
}

const int32_t *sdl_batch_position_ids(const sdl_batch *b) {
    if (!b || !b->owner_) return nullptr;
    const HostBatch *hb = static_cast<const HostBatch *>(b->owner_);
    return hb->tt_is_pos ? hb->tt : nullptr;
}

const int32_t *sdl_batch_pair_labels(const sdl_batch *b) {
    if (!b || !b->owner_) return nullptr;
    const HostBatch *hb = static_cast<const HostBatch *>(b->owner_);
    return hb->pair_lab.empty() ? nullptr : hb->pair_lab.data();
}

int sdl_process_device(sdl_batcher *h, const uint8_t *d_text, uint64_t text_len, const uint64_t *d_offsets,
                       uint64_t n_records, uint64_t first_record, void *stream, sdl_device_rows *out) {
    return sdl_process_device_labels(h, d_text, text_len, d_offsets, n_records, nullptr, nullptr, first_record, stream,
                                     out);
}

int sdl_process_device_labels(sdl_batcher *h, const uint8_t *d_text, uint64_t text_len, const uint64_t *d_offsets,
                              uint64_t n_records, const uint32_t *d_labels, const uint64_t *d_label_offsets,
                              uint64_t first_record, void *stream, sdl_device_rows *out) {
    if (!h || !out || !d_offsets || (!d_text && text_len)) return fail(SDL_ERR_ARG, "null argument");
    if (h->pair())
        return fail(SDL_ERR_STATE, "sdl_process_device[_labels] on a handle created with pair = 1: use sdl_process_device_pairs");
    return process_device_checked(h, d_text, text_len, d_offsets, n_records, n_records, d_labels, d_label_offsets,
                                  first_record, stream, out);
}

int sdl_process_device_pairs(sdl_batcher *h, const uint8_t *d_text, uint64_t text_len, const uint64_t *d_offsets,
                             uint64_t n_pairs, const uint32_t *d_labels, const uint64_t *d_label_offsets,
                             uint64_t first_record, void *stream, sdl_device_rows *out) {
    if (!h || !out || !d_offsets || (!d_text && text_len)) return fail(SDL_ERR_ARG, "null argument");
    if (!h->pair()) return fail(SDL_ERR_STATE, "sdl_process_device_pairs needs a handle created with pair = 1");
    if (n_pairs >= (1ull << 31)) return fail(SDL_ERR_CAPACITY, "too many pairs in one call");
    return process_device_checked(h, d_text, text_len, d_offsets, 2 * n_pairs, n_pairs, d_labels, d_label_offsets,
                                  first_record, stream, out);
}

int sdl_pack_flush_device(sdl_batcher *h, void *stream, sdl_device_rows *out) {
    if (!h || !out) return fail(SDL_ERR_ARG, "null argument");
    if (!h->pack()) return fail(SDL_ERR_STATE, "sdl_pack_flush_device needs a handle created with pack = 1");
    return guarded(SDL_ERR_ARG, SDL_ERR_ARG, [&]() -> int {
        h->run_pack_flush(stream ? (hipStream_t)stream : h->stream);
        std::memset(out, 0, sizeof(*out));
        out->input_ids = h->o_ids.p;
        out->attention_mask = h->o_am.p;
        out->labels = h->o_lab.p;
        out->d_rows = h->pk_meta.p;
        out->rows_capacity = (uint64_t)h->last_rows_cap;
        out->label_width = h->P.label_width;
        return SDL_OK;
    });
}

const int32_t *sdl_device_position_ids(sdl_batcher *h) { return h && h->pack() && h->pk_ran ? h->o_tt.p : nullptr; }

const int32_t *sdl_device_pair_labels(sdl_batcher *h) {
    return h && h->pair_mlm() && h->pair_lab_ran ? h->o_pair_lab.p : nullptr;
}

int sdl_tokenizer_info_get(const char *tokenizer_path, const char *data_dir, sdl_tokenizer_info *out) {
    if (!tokenizer_path || !out) return fail(SDL_ERR_ARG, "null argument");
    return guarded(SDL_ERR_IO, SDL_ERR_IO, [&]() -> int {  // (no HIP call in here: nothing maps to SDL_ERR_HIP)
        HostTokenizer t;
        load_tokenizer(tokenizer_path, data_dir ? std::string(data_dir) : default_data_dir(), t);
        std::memset(out, 0, sizeof(*out));
        out->kind = t.kind;
        out->vocab_size = (int32_t)t.pieces.size();
        out->n_added = (int32_t)t.added.size();
        out->unk_id = t.unk_id;
        out->eos_id = t.eos_id;
        int mx = 0;
        for (auto &p : t.pieces) mx = std::max(mx, (int)p.size());
        out->max_piece_bytes = mx;
        out->word_table_entries = t.kind == TOK_WORDPIECE ? 0 : t.word_table_entries;
        out->normalizer_flags = (t.cased ? 1 : 0) | (t.keeps_accents ? 2 : 0);
        return SDL_OK;
    });
}

int sdl_set_profiling(sdl_batcher *h, int enable) {
    if (!h) return fail(SDL_ERR_ARG, "null argument");
    h->profiling = enable != 0;
    return SDL_OK;
}

int sdl_stage_times(sdl_batcher *h, const char **names, float *ms, int cap) {
    if (!h) return fail(SDL_ERR_ARG, "null argument");
    if (!h->profiling) return fail(SDL_ERR_STATE, "profiling not enabled");
    if (hipEventSynchronize(h->ev[h->n_stages]) != hipSuccess) return fail(SDL_ERR_HIP, "event sync failed");
    int n = std::min(cap, h->n_stages);
    for (int i = 0; i < n; ++i) {
        float t = 0.f;
        if (hipEventElapsedTime(&t, h->ev[i], h->ev[i + 1]) != hipSuccess) return fail(SDL_ERR_HIP, "event time");
        if (names) names[i] = h->stage_names[i];
        if (ms) ms[i] = t;
    }
    return n;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// Several GPUs, one record stream (the reference runs one Batcher task,
// rust/src/tasks/runner_simple.rs:68-112): byte-balanced contiguous record ranges, one
// handle + stream + host thread per device, masks keyed by the global record index.
// ---------------------------------------------------------------------------
int sdl_shard_records(const uint64_t *offsets, uint64_t n_records, uint32_t n_shards, uint64_t *bounds) {
    if (!offsets || !bounds || n_shards == 0) return fail(SDL_ERR_ARG, "null argument or zero shards");
    for (uint64_t r = 0; r < n_records; ++r)
        if (offsets[r + 1] < offsets[r]) return fail(SDL_ERR_ARG, "offsets must be non-decreasing");
    const uint64_t base = offsets[0], total = offsets[n_records] - base;
    bounds[0] = 0;
    for (uint32_t k = 1; k < n_shards; ++k) {
        // the first record starting at or past k * total / n_shards
        const unsigned __int128 t = (unsigned __int128)total * k / n_shards;
        const uint64_t want = base + (uint64_t)t;
        bounds[k] = (uint64_t)(std::lower_bound(offsets, offsets + n_records, want) - offsets);
        if (bounds[k] < bounds[k - 1]) bounds[k] = bounds[k - 1];
    }
    bounds[n_shards] = n_records;
    return SDL_OK;
}

struct sdl_multi {
    std::vector<sdl_batcher *> h;
    uint64_t next_record = 0;  // global index of the next call's first record
    bool poisoned = false;     // a shard failed: the others committed their part of that push
    ~sdl_multi() {
        for (sdl_batcher *x : h) sdl_batcher_destroy(x);
    }
};

int sdl_multi_create(const sdl_config *cfg, const char *tokenizer_path, const char *data_dir, const int32_t *devices,
                     uint32_t n_devices, sdl_multi **out) {
    if (!cfg || !devices || !out || n_devices == 0) return fail(SDL_ERR_ARG, "null argument or no devices");
    if (cfg->pair == 1)
        return fail(SDL_ERR_UNSUPPORTED, "sdl_multi_create with pair = 1: sentence pairs are not sharded over several handles");
    if (cfg->pair >= SDL_PAIR_MLM && cfg->pair <= SDL_PAIR_MLM_SOP)
        return fail(SDL_ERR_UNSUPPORTED,
                    "sdl_multi_create with pair = 2..4: sentence pairs are not sharded over several handles (a next-"
                    "sentence draw is over one call's pairs)");
    std::unique_ptr<sdl_multi> m(new sdl_multi());
    m->next_record = cfg->first_record;
    for (uint32_t k = 0; k < n_devices; ++k) {
        sdl_config c = *cfg;
        c.device = devices[k];
        sdl_batcher *h = nullptr;
        if (int rc = sdl_batcher_create(&c, tokenizer_path, data_dir, &h)) return rc;
        m->h.push_back(h);
    }
    *out = m.release();
    return SDL_OK;
}

void sdl_multi_destroy(sdl_multi *m) { delete m; }

sdl_batcher *sdl_multi_handle(sdl_multi *m, uint32_t k) { return m && k < m->h.size() ? m->h[k] : nullptr; }

int sdl_multi_push_many(sdl_multi *m, const uint8_t *arena, const uint64_t *offsets, size_t n_records,
                        const uint32_t *labels, const uint64_t *label_offsets, size_t *n_emitted) {
    if (!m || !offsets || (!arena && n_records && offsets[n_records])) return fail(SDL_ERR_ARG, "null argument");
    if (offsets[0] != 0) return fail(SDL_ERR_ARG, "offsets must start at 0");
    if (m->poisoned) return fail(SDL_ERR_STATE, "an earlier push failed on a shard; the stream is not resumable");
    const uint32_t n = (uint32_t)m->h.size();
    std::vector<uint64_t> bounds(n + 1);
    if (int rc = sdl_shard_records(offsets, n_records, n, bounds.data())) return rc;
    std::vector<int> rcs(n, SDL_OK);
    std::vector<std::string> errs(n);
    std::vector<size_t> emitted(n, 0);
    auto run = [&](uint32_t k) {
        const uint64_t r0 = bounds[k], r1 = bounds[k + 1];
        sdl_batcher *h = m->h[k];
        if (hipSetDevice(h->device) != hipSuccess) {
            rcs[k] = SDL_ERR_HIP;
            errs[k] = "hipSetDevice failed";
            return;
        }
        std::vector<uint64_t> off(r1 - r0 + 1);
        for (uint64_t r = r0; r <= r1; ++r) off[r - r0] = offsets[r] - offsets[r0];
        h->first_override = (int64_t)(m->next_record + r0);
        rcs[k] = sdl_batcher_push_many(h, arena ? arena + offsets[r0] : nullptr, off.data(), (size_t)(r1 - r0), labels,
                                       label_offsets ? label_offsets + r0 : nullptr, &emitted[k]);
        h->first_override = -1;
        if (rcs[k] != SDL_OK) errs[k] = g_err;  // (the message is thread-local)
        // the handle's own counter follows its records; the next call's shard starts are global
    };
    std::vector<std::thread> th;
    for (uint32_t k = 1; k < n; ++k) th.emplace_back(run, k);
    run(0);
    for (auto &t : th) t.join();
    if (n_emitted)  // also on failure: the shards that succeeded have queued these
        for (uint32_t k = 0; k < n; ++k) n_emitted[k] = rcs[k] == SDL_OK ? emitted[k] : 0;
    for (uint32_t k = 0; k < n; ++k)
        if (rcs[k] != SDL_OK) {
            m->poisoned = true;
            return fail(rcs[k], "shard " + std::to_string(k) + ": " + errs[k]);
        }
    m->next_record += n_records;
    return SDL_OK;
}
