// handle.hpp -- what the host translation units behind the C ABI share (no .hip file includes
// this): the error types and the one error map, device / pinned buffers, the host batches, and
// struct sdl_batcher -- the batcher's own state as direct members (sdl_batcher.cpp), each
// provider step's buffers in a sub-struct of its own (provider_*.cpp, transport.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/sdl_batcher.h"
#include "assets.hpp"
#include "kernels.hpp"

namespace sdl {

inline thread_local std::string g_err;

inline int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) throw HipError(std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
struct ArgError : std::runtime_error { using std::runtime_error::runtime_error; };
struct CapacityError : std::runtime_error { using std::runtime_error::runtime_error; };

// The error map of every entry point: runs its body and turns what it throws into a status code,
// the message in sdl_last_error().  A HipError is SDL_ERR_HIP everywhere; the codes of a
// CapacityError and of any other std::exception (an ArgError too) are the entry point's own
// (DESIGN.md §0 lists them).
template <class F>
int guarded(int capacity, int other, F &&body) {
    try {
        return body();
    } catch (HipError &e) {
        return fail(SDL_ERR_HIP, e.what());
    } catch (CapacityError &e) {
        return fail(capacity, e.what());
    } catch (std::exception &e) {
        return fail(other, e.what());
    }
}

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;  // elements
    void ensure(size_t n) {
        if (n <= cap && p) return;
        if (p) (void)hipFree(p);
        p = nullptr;
        size_t want = std::max<size_t>(n + n / 4, 64);
        HIP_TRY(hipMalloc(&p, want * sizeof(T)));
        cap = want;
    }
    // a host table to the device, synchronously; returns the device pointer
    T *upload(const T *src, size_t n) {
        ensure(n);
        HIP_TRY(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        return p;
    }
    T *upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

template <class T>
struct PinBuf {
    T *p = nullptr;
    size_t cap = 0;
    void ensure(size_t n) {
        if (n <= cap && p) return;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        size_t want = std::max<size_t>(n + n / 4, 64);
        HIP_TRY(hipHostMalloc(&p, want * sizeof(T), hipHostMallocDefault));
        cap = want;
    }
    ~PinBuf() {
        if (p) (void)hipHostFree(p);
    }
};

// Pinned blocks holding finished batches, recycled: the device rows are copied
// straight into them (one D2H per plane per batch segment, no host re-copy),
// and a block returns here when its batch is released -- possibly after the
// handle is gone, so batches share ownership of the pool.
struct BatchPool {
    struct Block {
        void *host, *dev;  // dev: the device-mapped address (k_rows_to_host writes there)
    };
    std::mutex mu;
    std::vector<Block> free_;
    size_t bytes;
    size_t fresh = 0;  // blocks allocated so far
    explicit BatchPool(size_t b) : bytes(b) {}
    Block get() {
        {
            std::lock_guard<std::mutex> g(mu);
            if (!free_.empty()) {
                const Block b = free_.back();
                free_.pop_back();
                return b;
            }
        }
        Block b{nullptr, nullptr};
        HIP_TRY(hipHostMalloc(&b.host, bytes, hipHostMallocDefault));
        if (hipHostGetDevicePointer(&b.dev, b.host, 0) != hipSuccess) {
            (void)hipHostFree(b.host);
            throw HipError("hipHostGetDevicePointer failed");
        }
        std::lock_guard<std::mutex> g(mu);
        ++fresh;
        return b;
    }
    void put(const Block &b) {
        std::lock_guard<std::mutex> g(mu);
        free_.push_back(b);
    }
    ~BatchPool() {
        for (const Block &b : free_) (void)hipHostFree(b.host);
    }
};

// One DataSet being filled (BertData / GptData), planes in one pinned block.
// Rows [rows, B) get the initial values of BatchConfig::create_vector
// (batcher.rs:17-22) and BertData::new (bert_data.rs:27-38) when the batch is
// handed out (init_tail): filled rows are written once, by the D2H.
struct HostBatch {
    std::shared_ptr<BatchPool> pool;
    void *block = nullptr;
    char *dev = nullptr;  // the block's device-mapped address (k_rows_to_host writes there)
    int32_t *ids = nullptr, *am = nullptr, *tt = nullptr, *lab = nullptr;
    float *f32 = nullptr;  // MultiLabel: [B, number_labels]
    int rows = 0;
    int B, S, LW;
    bool tt_is_pos = false;  // pack = 1 (clm): the fourth plane holds position_ids, not token types
    // pair 2..4 (mlm): the pair label of every row, [B] (plain host memory: the cadence loop writes
    // it from the call's pair-label plane); empty otherwise
    std::vector<int32_t> pair_lab;
    static size_t block_bytes(int B, int S, int LW, bool with_tt) {
        return 4 * (size_t)B * ((size_t)S * (with_tt ? 3 : 2) + (size_t)LW);
    }
    HostBatch(std::shared_ptr<BatchPool> pl, int B_, int S_, int LW_, bool with_tt, bool multi)
        : pool(std::move(pl)), B(B_), S(S_), LW(LW_) {
        const BatchPool::Block bl = pool->get();
        block = bl.host;
        dev = static_cast<char *>(bl.dev);
        int32_t *q = static_cast<int32_t *>(block);
        const size_t BS = (size_t)B * S;
        ids = q;
        am = q + BS;
        q += 2 * BS;
        if (with_tt) {
            tt = q;
            q += BS;
        }
        if (multi) f32 = reinterpret_cast<float *>(q);
        else lab = q;
    }
    template <class T>
    int32_t *on_dev(T *host_plane) const {
        return host_plane ? reinterpret_cast<int32_t *>(dev + ((char *)host_plane - (char *)block)) : nullptr;
    }
    HostBatch(const HostBatch &) = delete;
    HostBatch &operator=(const HostBatch &) = delete;
    void init_tail() {
        const size_t r0 = (size_t)rows, r1 = (size_t)B;
        if (r0 >= r1) return;
        std::fill(ids + r0 * S, ids + r1 * S, 0);
        std::fill(am + r0 * S, am + r1 * S, 1);
        if (tt) std::fill(tt + r0 * S, tt + r1 * S, 0);  // (token types and position_ids alike)
        if (lab) std::fill(lab + r0 * LW, lab + r1 * LW, -100);
        if (f32) std::fill(f32 + r0 * LW, f32 + r1 * LW, 0.f);
        if (!pair_lab.empty()) std::fill(pair_lab.begin() + (long)r0, pair_lab.end(), -100);
    }
    ~HostBatch() { pool->put(BatchPool::Block{block, dev}); }
};

// memcpy of a large host buffer on several threads (pageable -> pinned staging)
inline void par_copy(void *dst, const void *src, size_t n) {
    const size_t kMin = (size_t)8 << 20;
    unsigned T = std::thread::hardware_concurrency();
    T = T < 1 ? 1 : T > 8 ? 8 : T;
    if (n < kMin || T == 1) {
        std::memcpy(dst, src, n);
        return;
    }
    const size_t per = (n / T + 4095) & ~(size_t)4095;
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) {
        const size_t a = per * t;
        if (a >= n) break;
        const size_t b = std::min(n, a + per);
        th.emplace_back([=] { std::memcpy((char *)dst + a, (const char *)src + a, b - a); });
    }
    std::memcpy(dst, src, std::min(n, per));
    for (auto &x : th) x.join();
}

// segments per call (SDL_SEGMENTS) and the fewest 1 KiB chunks a pipelined
// segment holds (SDL_SEG_MIN_CHUNKS, default 16 MiB of text); read when a
// handle is created
inline int env_int(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::max(1, std::atoi(e)) : dflt;
}
// the same for switches and values where 0 means something (env_int reads "0" as 1)
inline int env_int0(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e ? std::max(0, std::atoi(e)) : dflt;
}

// JsonText provider step (sdl_json_text_device); it also uses the handle's scan_tmp and pin_u32_2
struct JsonWork {
    DevBuf<uint32_t> cnt, base, nl, len, rec, toff, ridx, inv, tail;
    DevBuf<uint2> span;
    DevBuf<uint8_t> text;
    DevBuf<uint64_t> off;
};
// what sdl_inflated points to: gzip inflate and zstd decode both size, write and report here
struct InflatedOut {
    DevBuf<uint32_t> size, off, bad;
    DevBuf<int32_t> status;
    DevBuf<uint8_t> out;
};
// gzip inflate provider step (sdl_gzip_inflate_device)
struct InflateWork {
    DevBuf<uint32_t> tcrc;
    DevBuf<uint64_t> from, mend;  // (sdl_gzip_inflate_first_device) candidate search start, member ends
    DevBuf<unsigned long long> total;
};
// ... large members in chunks (inflate_chunked)
struct InflateChunkWork {
    DevBuf<uint64_t> nominal, found, start, hdr, end, endhdr, pos;
    DevBuf<uint32_t> list, tgt, next, len, flags, order, crc, shift, stats;
    DevBuf<int32_t> status, rstatus;
    DevBuf<uint16_t> slots;
    DevBuf<uint8_t> windows, gwin;
    DevBuf<uint16_t> gmaps;
};
// zstd frame decode provider step (sdl_zstd_inflate_device): frame and block records, the scans'
// inputs and outputs, the literal arena and the sequence records (outputs go to InflatedOut's out /
// off / status / bad)
struct ZstdWork {
    DevBuf<zs::Frame> frames;
    DevBuf<zs::Block> blocks;
    DevBuf<uint32_t> nblk, first, lit_tot, seq_tot, lit_base, seq_base;
    DevBuf<unsigned long long> totals;
    DevBuf<uint8_t> lit;
    DevBuf<zs::SeqRec> seq;
};
// Transport frames (sdl_pickle_frames_device)
struct FrameWork {
    DevBuf<uint8_t> out, out2;
    DevBuf<uint8_t> *target = &out;  // where the next frames go
    uint8_t *dest = nullptr;         // ... or here (device-visible, e.g. mapped pinned host memory)
    size_t dest_cap = 0;
    bool dry = false;                // lay the frames out, launch nothing
};
// sdl_json_to_frames: input slots, the rows carried between chunks, streams/events
struct JsonFramesWork {
    DevBuf<uint8_t> json[2], frames[2];
    PinBuf<uint8_t> pin_in[2], pin_out[2];
    DevBuf<int32_t> ids[2], am[2], tt[2], lab[2];
    hipStream_t in = nullptr, out = nullptr;
    hipEvent_t ev[8] = {};
    std::vector<hipEvent_t> in_ev;  // json_to_frames, pinned input: chunk k's H2D done
    DevBuf<uint8_t> json_all;       // ... every chunk, 32 zero bytes after each
};

constexpr int kStages = 7;
extern const char *kStageNames[];  // (sdl_batcher.cpp)

}  // namespace sdl

using namespace sdl;  // (this header serves the library's own host files only)

struct sdl_batcher {
    sdl_config cfg{};
    RowParams P{};
    HostTokenizer tok;
    DevTok dt{};
    DevFirst dfirst{};
    hipStream_t stream = nullptr;
    int device = 0;

    // device-resident tokenizer tables
    DevBuf<uint16_t> d_upage;
    DevBuf<uint32_t> d_uentry, d_ubmp;
    DevBuf<uint8_t> d_upool, d_vpool;
    DevBuf<VSlot> d_slots, d_wslots;
    DevBuf<int32_t> d_ascii_id;
    DevBuf<uint8_t> d_wp_lens;
    DevBuf<WfSlot> d_first_slots;
    DevBuf<uint32_t> d_cont_bits;  // mask policy 2: the continuation bitmap (HostTokenizer::cont_bits)
    MaskPolicy mpol{};             // sdl_config.mask_policy / mask_per_mille, as k_rows_policy takes them
    DevBuf<uint16_t> d_gpage, d_byte_id;
    DevBuf<uint8_t> d_gblock;
    DevBuf<MSlot> d_mslots;
    // unigram (t5)
    DevBuf<double> d_uscore;
    DevBuf<uint16_t> d_wres, d_cpage;
    DevBuf<uint8_t> d_upfx;
    DevBuf<uint2> d_cent, d_cbmp;
    DevBuf<float> d_uscore32;
    DevBuf<uint8_t> d_tnorm;
    DevBuf<uint32_t> d_trie;
    DevBuf<int32_t> d_extra;
    DevBuf<double> d_zig;  // span rng_mode 1: ZIG_NORM_X then ZIG_NORM_F (257 each)
    DevBuf<uint32_t> d_span_counts;  // span policy 1: t | m << 16 for every n in 0..S (span_noise_table)
    SpanNoise snoise{};              // ... as k_rows_span_t5 takes it; counts null = the reference's rule

    // per-call workspace
    DevBuf<uint32_t> row_chunk;  // row -> the chunk of its first id (rows read from the chunk lists)
    DevBuf<uint32_t> ranges, tokc, chunk_cnt, chunk_off, rec_local, tok_ids, rec_tok, rec_cnt, rec_rows, row_off,
        row_rec, scan_tmp;
    DevBuf<int32_t> o_ids, o_am, o_tt, o_lab;
    // rng_mode 1: the swap indices and mask bits of the rows walked beside the tokenizer on stream2
    // (k_mask_rand_rec: chunk 0 of every record, chunk 1 of the spec_list records); k_rows walks the
    // rest in a second pass
    DevBuf<uint16_t> mask_j0;
    DevBuf<uint32_t> mask_bits0, spec_list, spec_pos;
    hipEvent_t rand_ev[4] = {nullptr, nullptr, nullptr, nullptr};
    DevBuf<float> o_f32;
    DevBuf<uint32_t> lab_err;
    // byte-level BPE long pieces
    DevBuf<uint32_t> long_count, chunk_ent;
    DevBuf<BpeLong> long_list;
    DevBuf<uint16_t> long_scratch;
    // unigram long items
    DevBuf<uint32_t> uni_counters, uni_pool, uni_err, span_err;
    // span rows in two phases: per-row pass plans, row meta, overflow rows
    DevBuf<uint2> span_tab, span_meta;
    DevBuf<uint32_t> span_ovf;
    bool span_two_phase = env_int0("SDL_SPAN_TWO_PHASE", 0) != 0;
    // rng_mode 1: chunk-0 rows walked beside the tokenizer (0: every row by its k_rows wave)
    bool rand_rec0 = env_int0("SDL_RAND_REC0", 1) != 0;
    // ... and chunk 1 of records of >= (S - frame + 1) / rho bytes (WordPiece/BPE give ~0.2-0.3 ids
    // per byte; SDL_RAND_SPEC_RHO_PCT=0: chunk 0 only)
    double rand_spec_rho = env_int0("SDL_RAND_SPEC_RHO_PCT", 25) / 100.0;
    // test hook: clamp the Unigram long-item list (0 = its N / 8 + chunks bound), so the capacity
    // flag can be raised through every path that reports it
    uint32_t uni_item_cap = (uint32_t)std::max(0, env_int0("SDL_UNI_ITEM_CAP", 0));
    DevBuf<uint4> uni_items, uni_items2, uni_huge;
    DevBuf<uint8_t> uni_scratch;
    // the provider steps' buffers, by owner (they share the stream, scan_tmp and the pinned words below)
    JsonWork json; InflatedOut inf; InflateWork gz; InflateChunkWork gzc; ZstdWork zs;
    FrameWork frames; JsonFramesWork jf;

    // host streaming path (GenTokenizer.store + emitted batches)
    std::deque<HostBatch *> store;
    std::deque<HostBatch *> outbox;
    PinBuf<uint8_t> pin_blob;  // staged call input: text | offsets | labels | label offsets
    // a small push's H2D done by k_chunk_ranges from the mapped blob (process_host -> run_device)
    struct FusedH2D {
        const void *src = nullptr;
        void *dst = nullptr;
        size_t bytes = 0;
        const uint64_t *h_off = nullptr;  // the offsets in the mapped blob
    } fused_h2d;
    void *blob_dev = nullptr;               // pin_blob's device address ...
    const uint8_t *blob_dev_host = nullptr;  // ... for this host buffer
    DevBuf<uint8_t> h2d_blob;
    PinBuf<uint32_t> pin_u32;
    PinBuf<uint32_t> pin_stat;  // direct pass: row offsets + error words (mapped)
    uint32_t *stat_dev = nullptr;
    HostBatch *spare = nullptr;  // direct pass: the next batch, allocated ahead
    DirectDst fuse_dd{};          // ... its destinations, for run_device's fused small path
    uint32_t *fuse_stat = nullptr;
    bool fused_done = false;      // run_device wrote the direct rows and the row offsets
    PinBuf<RowSeg> seg_pin;
    DevBuf<RowSeg> seg_dev;
    void ensure_stat(size_t n) {
        const uint32_t *was = pin_stat.p;
        pin_stat.ensure(n);
        if (pin_stat.p != was || !stat_dev) {
            void *d = nullptr;
            HIP_TRY(hipHostGetDevicePointer(&d, pin_stat.p, 0));
            stat_dev = static_cast<uint32_t *>(d);
        }
    }
    uint32_t pin_u32_err = 0;
    uint32_t pin_u32_2[2] = {0, 0};
    uint64_t n_records = 0;
    int64_t first_override = -1;  // sdl_multi: the global index of the next call's first record

    bool profiling = false;
    hipEvent_t ev[kStages + 1] = {};
    float stage_ms[kStages] = {};
    int n_stages = kStages;
    const char **stage_names = kStageNames;
    // pipelined segments: second stream, cross-stream events, record bounds
    hipStream_t stream2 = nullptr;
    hipStream_t stream_u = nullptr;  // unigram: the wide-job Viterbi and the long items beside the narrow jobs
    hipEvent_t uni_ev[2] = {nullptr, nullptr};
    std::vector<hipEvent_t> pipe_ev;
    DevBuf<uint32_t> seg_rb;
    int seg_target = env_int("SDL_SEGMENTS", 1);
    int64_t seg_min_chunks = env_int("SDL_SEG_MIN_CHUNKS", 16384);

#ifdef SDL_STAMPS
    ~sdl_batcher() {
        print_phase_cycles();
        print_uni_cycles();
        print_long_cycles();
        print_vit_cycles();
        print_bpe_cycles();
        if (uni_counters.p) {
            uint32_t c[4] = {0, 0, 0, 0}, e = 0;
            if (hipMemcpy(c, uni_counters.p, 16, hipMemcpyDeviceToHost) == hipSuccess &&
                hipMemcpy(&e, uni_err.p, 4, hipMemcpyDeviceToHost) == hipSuccess)
                fprintf(stderr, "[uni] long items %u, pool words %u, huge %u, err %u\n", c[0], c[2], c[3], e);
        }
        cleanup();
    }
    void cleanup() {
#else
    ~sdl_batcher() {
#endif
        for (auto *b : store) delete b;
        for (auto *b : outbox) delete b;
        delete spare;
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : pipe_ev) (void)hipEventDestroy(e);
        for (auto &e : rand_ev)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : jf.ev)
            if (e) (void)hipEventDestroy(e);
        for (auto &e : jf.in_ev) (void)hipEventDestroy(e);
        if (jf.in) (void)hipStreamDestroy(jf.in);
        if (jf.out) (void)hipStreamDestroy(jf.out);
        if (stream2) (void)hipStreamDestroy(stream2);
        for (auto &e : uni_ev)
            if (e) (void)hipEventDestroy(e);
        if (stream_u) (void)hipStreamDestroy(stream_u);
        if (stream) (void)hipStreamDestroy(stream);
    }

    bool multi() const { return P.task == SDL_TASK_MULTI_LABEL; }
    bool single() const { return P.task == SDL_TASK_SINGLE_CLASS; }
    bool simple() const { return multi() || single(); }  // SimpleBatcher (simple_batcher.rs)
    bool span() const { return P.task == SDL_TASK_SPAN; }
    bool with_tt() const { return P.task == SDL_TASK_MLM || simple(); }
    // sdl_config.pack = 1: clm rows cut from the concatenated document stream (pack.hip).  The
    // position_ids travel through the token-type plumbing clm does not use (o_tt, RowSeg.tt,
    // HostBatch.tt); the public token_type_ids stays NULL
    bool pack() const { return cfg.pack == 1; }
    bool plane4() const { return with_tt() || pack(); }
    // sdl_config.pair != 0: a call's 2 n text ranges are n examples of two texts, one row each
    // (pair = 1: pair.hip, the label tasks; pair 2..4: pair_mlm.hip, mlm with a drawn pair label)
    bool pair() const { return cfg.pair != 0; }
    bool pair_mlm() const { return cfg.pair >= SDL_PAIR_MLM; }

    std::shared_ptr<BatchPool> pool;
    HostBatch *new_batch() {
        if (!pool) pool = std::make_shared<BatchPool>(HostBatch::block_bytes(P.B, P.S, P.label_width, plane4()));
        HostBatch *b = new HostBatch(pool, P.B, P.S, P.label_width, plane4(), multi());
        b->tt_is_pos = pack();
        if (pair_mlm()) b->pair_lab.assign((size_t)P.B, -100);
        return b;
    }

    // pack = 1: the carry between calls, double buffered (ids and position_ids, S each per half),
    // and pk_meta = {rows of the last call, length of half 0, length of half 1}; the host only
    // knows which half is current -- it flips per call, the lengths stay on the device
    DevBuf<int32_t> pk_carry;
    DevBuf<uint32_t> pk_meta, pk_off;
    int pk_cur = 0;
    bool pk_ran = false;
    int64_t last_segments = 1;
    int64_t last_rows_cap = 0, last_R = 0;
    // (defined in sdl_batcher.cpp)
    PackParams pack_params(int64_t R, int64_t rows_cap);
    void run_pack(int64_t R, int64_t rows_cap, hipStream_t st);
    void run_pack_flush(hipStream_t st);
    DevBuf<uint32_t> pair_rb;  // pair != 0: the one segment's record bounds {0, n_pairs}
    DevBuf<int32_t> o_pair_lab;  // pair 2..4: the pair label of every row of the last call, grown with the row planes
    bool pair_lab_ran = false;   // ... written by a call (sdl_device_pair_labels is NULL before)
    PinBuf<int32_t> pin_pair_lab;  // host path: the call's pair labels beside its row offsets
    void run_pair(int64_t R, int64_t rows_cap, int64_t n_chunks, const uint64_t *d_off, uint64_t first_record,
                  hipStream_t st, const uint32_t *d_labels, const uint64_t *d_label_off);
    int64_t rows_capacity(int64_t N, int64_t R) const;
    void run_device(const uint8_t *d_text, int64_t N, const uint64_t *d_off, int64_t R, uint64_t first_record,
                    hipStream_t st, const uint32_t *d_labels = nullptr, const uint64_t *d_label_off = nullptr);
    void ensure_pipe_events(int K);
    void ensure_stream2();
    void queue_packed_rows();
    void process_host(const uint8_t *arena, const uint64_t *offsets, int64_t R, const uint32_t *labels,
                      const uint64_t *label_off);
};
