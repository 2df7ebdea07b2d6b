/*
 * sdl_batcher.h -- C ABI of the MI355X-native Batcher (libsdl_batcher.so).
 *
 * Drop-in boundary for the reference's Batcher stage
 * (andywag/streaming_data_loader @ v1, rust/src/batcher.rs:26-31):
 *
 *     pub trait Batcher { type S; type T;
 *         fn create_sync_batch(&mut self, data: Self::S) -> Option<Self::T>;
 *         fn get_working_batch(&mut self) -> Option<Self::T>; }
 *
 * implemented for the masking tasks by GenTokenizer
 * (rust/src/tasks/gen_batcher.rs:65-98, S = String, T = DataSet) and for the
 * multi-label task by SimpleBatcher (rust/src/models/simple_batcher.rs:31-53).
 * INTEGRATION.md shows the Rust `impl Batcher for GpuBatcher` that binds this
 * header through `extern "C"` so the Provider -> Batcher -> Transport channels
 * (rust/src/tasks/runner_simple.rs:68-112) stay unchanged.
 *
 * Conventions: plain pointers and sizes only; every call returns an int
 * status (SDL_OK = 0, < 0 error; never a panic across the FFI; the message is
 * in sdl_last_error()).  One handle per host thread / GPU; handles are not
 * thread-safe.  Input text is copied in (the caller keeps ownership, as the
 * reference moves the String in); batches are owned by the handle until
 * sdl_batch_release().
 */
#ifndef SDL_BATCHER_H
#define SDL_BATCHER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 9 still: sdl_zstd_split_frames, sdl_zstd_inflate_device, the three sentence-pair calls and the
 * two pair-label accessors were added without changing any existing call or struct (an additive
 * change keeps the version). */
#define SDL_ABI_VERSION 9

enum {
    SDL_OK = 0,
    SDL_ERR_ARG = -1,         /* bad argument / config (reference: panic!/todo!) */
    SDL_ERR_IO = -2,          /* tokenizer asset unreadable */
    SDL_ERR_HIP = -3,         /* HIP runtime error */
    SDL_ERR_UNSUPPORTED = -4, /* task / tokenizer feature not implemented */
    SDL_ERR_NODEV = -5,       /* no HIP device: the product never falls back to the CPU */
    SDL_ERR_STATE = -6,       /* call out of order */
    SDL_ERR_CAPACITY = -7,    /* input larger than one call supports (>= 4 GiB of text) */
    SDL_ERR_DATA = -8         /* corrupt input the reference's unwrap() panics on (gzip, zstd) */
};

/* TaskType -> DataSet selection (rust/src/config.rs:20-62). */
enum {
    SDL_TASK_MLM = 0,        /* BertData, DataSetConfig::Mask   (models/bert_data.rs) */
    SDL_TASK_CLM = 1,        /* GptData,  DataSetConfig::Gpt    (models/gpt_data.rs) */
    SDL_TASK_SPAN = 2,       /* T5Data,   DataSetConfig::Span   (models/t5_data.rs) */
    SDL_TASK_MULTI_LABEL = 3, /* BertData, DataSetConfig::MultiLabel via SimpleBatcher */
    SDL_TASK_SINGLE_CLASS = 4 /* BertData, DataSetConfig::SingleClass via SimpleBatcher
                                 (tasks/single_class/runner.rs:40-49): one Label::Single per record */
};

/* Mirrors TrainingConfig.batch + .dataset_config (rust/src/config.rs:64-72,
 * rust/src/batcher.rs:11-14, rust/src/datasets/dataset_config.rs:7-16) plus the
 * RNG seed that replaces the reference's unseedable thread_rng().  96 bytes; the last three words
 * are a C11 anonymous union (reserved[3], kept for callers that zero it, and the span policy's two
 * words over reserved[0] and reserved[1]). */
struct sdl_config {
    int32_t task;            /* SDL_TASK_* */
    int32_t batch_size;      /* BatchConfig.batch_size */
    int32_t sequence_length; /* BatchConfig.sequence_length */
    int32_t chunk;           /* GenTokenizer.chunk (1 for the masking tasks, masking_runner.rs:55-62) */
    int32_t min_ids;         /* records with fewer framed ids are dropped (gen_batcher.rs:74): 64 */
    int32_t mask_length;     /* DataSetConfig::Mask.mask_length = (S as f32 * 0.15) as usize */
    int32_t mask_id;         /* DataSetConfig::Mask.mask = 103 (masking_cases.rs:60) */
    int32_t number_labels;   /* DataSetConfig::MultiLabel.number_labels */
    double avg_span_gap;     /* DataSetConfig::Span.avg_span_gap  (16.0) */
    double avg_span_size;    /* DataSetConfig::Span.avg_span_size (2.0) */
    uint64_t seed;           /* RNG contract seed */
    uint64_t first_record;   /* global index of this handle's first record (sharding) */
    int32_t device;          /* HIP device ordinal */
    int32_t rng_mode;        /* 0 = the Philox contract (default);
                                1 = the reference's own draws on a per-row StdRng::from_seed(
                                seed | record | chunk, little-endian, zero padded):
                                MLM masks = rand 0.8.5 position_base.shuffle (bert_data.rs:40-43;
                                S <= 2048); span gap / size = rand_distr 0.4.3 StandardNormal,
                                gap then size per pass (t5_data.rs:165-176) */
    int32_t mask_policy;     /* SDL_MASK_*: which positions of an MLM row are masked and what replaces
                                them (DESIGN.md §3 "Masking policies").  0 = the reference's rule */
    int32_t mask_per_mille;  /* policies 1 and 2: predictions per 1000 filled positions of a row (150);
                                mask_length stays the row's maximum.  Ignored under policy 0 */
    int32_t pack;            /* CLM, byte-level BPE: 0 = GenTokenizer's rows (every record cut into its own
                                rows); 1 = documents concatenated with the end-of-text id and the stream
                                cut into full rows ("Packed rows" below).  Carved out of reserved[4] */
    union {                  /* the last three words under two views: a zeroed config is the reference's */
        int32_t reserved[3];
        struct {
            int32_t span_policy;          /* SDL_SPAN_*: what a span row does with its ids (DESIGN.md §3
                                             "Span policies").  0 = the reference's rule */
            int32_t span_noise_per_mille; /* policy 1: noise ids per 1000 ids of a row (T5: 150), 1..500;
                                             sdl_config_default leaves it 0, the caller states it */
            int32_t pair;                 /* SDL_PAIR_*, WordPiece: 0 = one text per record; 1 = two texts per
                                             example in one [CLS] A [SEP] B [SEP] row (single-class /
                                             multi-label); 2..4 = that row under mlm with a BERT masking
                                             policy and a pair label ("Sentence pairs" below).  Other
                                             values are refused */
        };
    };
};
typedef struct sdl_config sdl_config;

/* sdl_config.span_policy (task span, rng_mode 0).  Policy 1 is T5's random_spans_noise_mask: a row
 * of n ids has t = min(max((n * span_noise_per_mille + 500) / 1000, 1), n - 1) noise ids in
 * m = min(max(1, floor(t / avg_span_size + 0.5)), t, n - t) spans (avg_span_size is the mean noise
 * span length, T5: 3.0; avg_span_gap is ignored; n < 2: t = m = 0), both cut by uniformly random
 * compositions; input_ids holds each span's kept ids and its sentinel, labels each sentinel and
 * its noise ids and a closing sentinel, attention_mask is 1 over the filled input positions only.
 * sdl_batcher_create refuses a config whose full row needs more than S/4 labels or 100 sentinels. */
enum {
    SDL_SPAN_REFERENCE = 0, /* T5Data::put_data: gaps and sizes drawn pass by pass */
    SDL_SPAN_T5 = 1         /* fixed noise density, fixed span count, uniform span boundaries */
};

/* sdl_config.mask_policy (MLM, rng_mode 0).  The two BERT policies never pick 0, mask_id or the
 * framing ids ([CLS], [SEP]); they pick k = min(mask_length, max(1, (l * mask_per_mille + 500) /
 * 1000)) of a row's l filled positions and replace 80 % by mask_id, 10 % by a uniform random id
 * below the vocabulary size and leave 10 % (labels carry the id at every picked position).
 * Both were carved out of reserved[6]: a zeroed field is the reference's rule, as before. */
enum {
    SDL_MASK_REFERENCE = 0,       /* BertData::mask_batch: mask_length draws of 0..S, non-zero ids -> mask_id */
    SDL_MASK_BERT = 1,            /* BERT's create_pretraining_data.py, token by token */
    SDL_MASK_BERT_WHOLE_WORD = 2  /* ... whole words: a WordPiece continuation piece ("##...") goes with
                                     the piece before it; a word that no longer fits is skipped */
};

/* A finished batch: DataSet's Serialize view (bert_data.rs:106-145,
 * gpt_data.rs:53-62, t5_data.rs:235-249) as int32 row-major planes. */
typedef struct sdl_batch {
    int32_t rows;            /* rows filled (BertData.index); the MLM `labels` list has this length */
    int32_t batch_size;
    int32_t sequence_length;
    int32_t label_width;     /* S (mlm/clm), S/4 (span), number_labels (multi-label), 1 (single-class) */
    const int32_t *input_ids;      /* [batch_size, sequence_length] */
    const int32_t *attention_mask; /* [batch_size, sequence_length] */
    const int32_t *token_type_ids; /* [batch_size, sequence_length] or NULL (clm/span) */
    const int32_t *labels;         /* [batch_size, label_width] or NULL (multi-label); single-class:
                                      [batch_size, 1], the BertData `label` list = the first `rows` */
    const float *labels_f32;       /* [batch_size, number_labels] (multi-label) or NULL */
    void *owner_;                  /* opaque, for sdl_batch_release */
} sdl_batch;

typedef struct sdl_batcher sdl_batcher;

/* ---- Packed rows (sdl_config.pack = 1; task clm, byte-level BPE) -----------
 * No counterpart in the reference (like mask_policy): what GPT-2/3, Megatron and the HF
 * group_texts recipes train on.  With t_r the tokenizer ids of record r (n_r of them, no
 * framing), record r is kept when n_r >= 1 and n_r + 1 >= min_ids (min_ids = 0 keeps every
 * non-empty document).  One call's stream is
 *     carry ++ concat over kept r of (t_r ++ [eos])         eos = sdl_tokenizer_info.eos_id
 * where carry is what the previous call on the handle left (< S ids, empty at first).  A stream of
 * L ids gives G = L / S rows, row g = stream[g S, (g + 1) S), and stream[G S, L) is the new carry.
 * Every emitted row has input_ids = labels = the stream ids (unshifted, as GptData) and
 * attention_mask 1 everywhere.  A fourth plane, position_ids, restarts at 0 at the start of each
 * row and after each document's eos (the eos belongs to its document): consumers derive
 * cu_seqlens from position_ids == 0 where attention_mask == 1.  Document ends come from the record
 * offsets, never from ids equal to eos, so a record holding the literal end-of-text string is
 * still one document.  A flush turns a carry of c > 0 ids into one more row in the plain
 * orientation -- columns < c as above, columns >= c input_ids 0, attention_mask 0, labels -100,
 * position_ids 0 (not the reversed range of the reference's unpacked attention_mask) -- and
 * empties the carry.  Rows from *d_rows to the next multiple of B hold the clm padding rows'
 * initial values with position_ids 0.  d_record_rows[r] is the number of stream positions record r
 * added (n_r + 1, or 0 when dropped); first_record and the seed are unused.
 * Host path: sdl_batcher_push_many queues every full batch a call completes, in order;
 * sdl_batcher_push is push_many of one record and returns the front of that queue (at most one
 * batch; the rest wait for sdl_batcher_next); sdl_batcher_flush first turns a non-empty carry
 * into the flush row, then pops the front of the queue -- full batches first, the partial one
 * last -- and returns 0 once no filled row is left.  sdl_batch.token_type_ids stays NULL.
 * sdl_multi_*: each shard's handle packs its own records, so packed rows, unlike unpacked ones,
 * are not the rows one handle gives over the whole stream.  sdl_json_to_frames returns
 * SDL_ERR_UNSUPPORTED; sdl_pickle_frames_device frames a packed call's three reference keys. */

/* ---- Sentence pairs (sdl_config.pair = 1; tasks single-class and multi-label, WordPiece) ----
 * No counterpart in the reference (SimpleData.alt_text is tokenized and dropped, dataset.rs:47):
 * what BERT-style classifiers are fine-tuned on (MNLI, QQP, QNLI, MRPC).  Example r is two texts
 * A_r, B_r with tokenizer ids a, b (n_a, n_b of them, no special tokens).  With M = S - 3 the kept
 * lengths (k_a, k_b) are those of tokenizers' longest_first truncation (right, stride 0):
 *     n_a + n_b <= M: (n_a, n_b);  else lo = min, hi = max of the two,
 *     hi = lo > M ? lo : max(lo, M - lo);  lo + hi > M: lo = M / 2, hi = M / 2 + M % 2;
 *     (k_a, k_b) = n_a <= n_b ? (lo, hi) : (hi, lo)          (a tie: B gets the odd id)
 * and the one row of the pair is
 *     input_ids       [CLS] a[0..k_a) [SEP] b[0..k_b) [SEP] 0 ...
 *     token_type_ids    0       0       0       1       1   0 ...
 *     attention_mask    1       1       1       1       1   0 ...      (the plain orientation)
 * -- what tokenizers' encode(A, B) gives under BertProcessing, truncated and padded to S.  An empty
 * A or B is legal; there is no min_ids filter and no chunking: exactly one row per pair.  Labels
 * are the task's, one set per pair.  Rows from *d_rows to the next multiple of B hold the unpaired
 * task's initial values.  sequence_length >= 3.  A pair handle takes sdl_process_device_pairs,
 * sdl_batcher_push_pair and sdl_batcher_push_many_pairs (sdl_batcher_next / _flush /
 * sdl_pickle_frames_device as they are); the unpaired calls return SDL_ERR_STATE on it and the
 * pair calls SDL_ERR_STATE on a handle with pair = 0.  sdl_json_to_frames and sdl_multi_create
 * return SDL_ERR_UNSUPPORTED.
 *
 * MLM rows and the NSP / SOP draw (pair = 2..4; task mlm, mask_policy 1 or 2, rng_mode 0, WordPiece,
 * 3 <= sequence_length <= 2048): what BERT and ALBERT pre-train on.  A call's 2 n text ranges are
 * n examples as above; `chunk` and `min_ids` are ignored, there is exactly one row per example, and
 * every row carries a sentence-level pair label.  Example r of a call over n_pairs examples has
 * global index rec = first_record + r and takes one Philox4x32-10 block, counter
 * (0, 0x70000000, rec lo, rec hi), key (seed lo, seed hi), words x, y, z, w:
 *     pair = 2 (SDL_PAIR_MLM)      first segment A_r, second B_r, pair label 0
 *     pair = 3 (SDL_PAIR_MLM_NSP)  random = x >= 0x80000000 && n_pairs >= 2; if random the second
 *                                  segment is B_s, s = j + (j >= r), j = umulhi(y, n_pairs - 1)
 *                                  (uniform over the other examples of the same call), else B_r;
 *                                  pair label = random (HF next_sentence_label: 0 = B continues A)
 *     pair = 4 (SDL_PAIR_MLM_SOP)  swap = x >= 0x80000000; if swap the first segment is B_r and the
 *                                  second A_r; pair label = swap (HF sentence_order_label)
 * The NSP draw depends on how the stream is cut into calls: a call is one API call (the host
 * calls hand a pair call to the device whole, never in parts), a foreign B comes from the same
 * call, and a call of one pair is never random.  Keeping B_s out of A_r's document is the caller's
 * job: put one document's pairs in different calls, or accept the noise as RoBERTa's ablation does.
 * The unmasked row is the pair row above of the two chosen segments (kept lengths from the chosen
 * sides' id counts, token types, the plain attention mask).  The masking is the mask_policy
 * contract applied to that row as chunk 0 of record rec -- the row's own index, also when its
 * second segment is foreign: candidates are the filled positions whose id is none of 0, mask_id,
 * [CLS], [SEP]; k = min(mask_length, max(1, (l * mask_per_mille + 500) / 1000)) with
 * l = k_a + k_b + 3, 0 without a candidate; keys, whole-word units, the 80/10/10 split and the
 * random ids as for unpaired rows.  labels is [rows, S], -100 off the picks; the pair labels are an
 * int32 plane of their own (sdl_device_pair_labels, sdl_batch_pair_labels).  Rows from *d_rows to
 * the next multiple of B hold the unpaired mlm initial values (ids 0, attention 1, token types 0,
 * labels -100) and pair label -100.  Label arguments of the pair calls are ignored.
 * sdl_batcher_push_pair works under pair 2 and 4 and returns SDL_ERR_UNSUPPORTED under pair 3 (a
 * call of one pair has nobody to draw from).  sdl_pickle_frames_device adds a fifth, flat key of
 * the frame's filled rows after the four mlm keys: "next_sentence_label" under pair 2 and 3,
 * "sentence_order_label" under pair 4. */
enum {
    SDL_PAIR_NONE = 0,    /* one text per record */
    SDL_PAIR_ROWS = 1,    /* single-class / multi-label: [CLS] A [SEP] B [SEP] rows */
    SDL_PAIR_MLM = 2,     /* mlm: pairs as given, pair label 0 everywhere */
    SDL_PAIR_MLM_NSP = 3, /* mlm: next-sentence draws */
    SDL_PAIR_MLM_SOP = 4  /* mlm: sentence-order draws */
};

/* Defaults of the reference masking cases (masking_cases.rs:38-94) for `task`:
 * B=4096 S=128 chunk=1 min_ids=64 mask 15%/103, span 16.0/2.0, 9 labels. */
void sdl_config_default(sdl_config *cfg, int32_t task);

/* get_tokenizer(cfg) + GenTokenizer::new / SimpleBatcher::new
 * (tokenizer_wrapper.rs:162-189, gen_batcher.rs:23-41).  `tokenizer_path` is a
 * HF tokenizer.json (or a WordPiece vocab.txt); `data_dir` holds the Unicode
 * tables (NULL = directory of the library's package data). */
int sdl_batcher_create(const sdl_config *cfg, const char *tokenizer_path, const char *data_dir,
                       sdl_batcher **out);
void sdl_batcher_destroy(sdl_batcher *h);

/* Batcher::create_sync_batch(data) for one record (gen_batcher.rs:69-94 /
 * simple_batcher.rs:35-43).  `labels` are the Label::Multi indices for the
 * multi-label task (ignored otherwise).  Returns 1 and fills *out when this
 * call emits a batch (at most one per call, as the reference), 0 when not. */
int sdl_batcher_push(sdl_batcher *h, const uint8_t *utf8, size_t len, const uint32_t *labels,
                     size_t n_labels, sdl_batch *out);

/* Bulk create_sync_batch over n_records records laid out back to back in
 * `arena` (record r = arena[offsets[r] .. offsets[r+1]), offsets[0] = 0,
 * n_records+1 offsets).  Exactly the batches the reference would emit over the
 * same sequence of calls are queued, in order, for sdl_batcher_next().  For the
 * multi-label task record r's Label::Multi indices are
 * labels[label_offsets[r] .. label_offsets[r+1]) (NULL label_offsets = none). */
int sdl_batcher_push_many(sdl_batcher *h, const uint8_t *arena, const uint64_t *offsets,
                          size_t n_records, const uint32_t *labels, const uint64_t *label_offsets,
                          size_t *n_emitted);
/* Pops the next batch queued by sdl_batcher_push_many: 1 = *out filled, 0 = none. */
int sdl_batcher_next(sdl_batcher *h, sdl_batch *out);
/* pair = 1: create_sync_batch for one example of two texts (either may be empty); labels as
 * sdl_batcher_push.  Returns 1 and fills *out when this call emits a batch (every B-th pair). */
int sdl_batcher_push_pair(sdl_batcher *h, const uint8_t *a, size_t len_a, const uint8_t *b, size_t len_b,
                          const uint32_t *labels, size_t n_labels, sdl_batch *out);
/* pair = 1: sdl_batcher_push_many over n_pairs examples: A_r is text range 2r and B_r range 2r+1
 * of `arena` (2 * n_pairs + 1 offsets); pair r's labels are labels[label_offsets[r] ..
 * label_offsets[r+1]) (n_pairs + 1 label offsets). */
int sdl_batcher_push_many_pairs(sdl_batcher *h, const uint8_t *arena, const uint64_t *offsets, size_t n_pairs,
                                const uint32_t *labels, const uint64_t *label_offsets, size_t *n_emitted);
/* Batcher::get_working_batch() (gen_batcher.rs:96-98): pops the front batch
 * (possibly partial, possibly empty).  1 = *out filled, 0 = none left. */
int sdl_batcher_flush(sdl_batcher *h, sdl_batch *out);
void sdl_batch_release(sdl_batch *b);
/* pack = 1: the batch's position_ids plane [batch_size, sequence_length] (owned like the other
 * planes); NULL for an unpacked batch. */
const int32_t *sdl_batch_position_ids(const sdl_batch *b);
/* pair = 2..4: the batch's pair labels [batch_size], the first `rows` filled, -100 above (owned like
 * the other planes: valid until sdl_batch_release); NULL for any other batch. */
const int32_t *sdl_batch_pair_labels(const sdl_batch *b);

/* ---- Device-resident bulk path (the measured hot path) -------------------
 * Tokenize + label every record of a device-resident arena in one sequence of
 * kernel launches on `stream` (a hipStream_t; NULL = the handle's stream),
 * without any host synchronisation.  Rows are packed densely in record order:
 * batch b is rows [b*B, (b+1)*B); rows >= *d_rows up to the next multiple of B
 * hold the reference's initial values.  Buffers are owned by the handle and
 * stay valid until the next call.  The global record index of record r (RNG
 * key) is first_record + r. */
typedef struct sdl_device_rows {
    int32_t *input_ids;      /* device [rows_capacity, S] */
    int32_t *attention_mask; /* device [rows_capacity, S] */
    int32_t *token_type_ids; /* device [rows_capacity, S] or NULL */
    int32_t *labels;         /* device [rows_capacity, label_width] */
    float *labels_f32;       /* device [rows_capacity, number_labels] or NULL */
    uint32_t *d_rows;        /* device scalar: rows produced */
    uint32_t *d_record_rows; /* device [n_records]: rows each record produced */
    uint32_t *d_tokens;      /* device scalar: tokenizer ids produced (before framing) */
    uint64_t rows_capacity;
    int32_t label_width;
    uint32_t *d_label_errors; /* device scalar: multi-label -- Label::Multi indices >= number_labels
                                 that were skipped; span -- label writes past the S/4 label width or
                                 sentinel indices >= 100 that were clamped (the reference panics on
                                 both: bert_data.rs:70-72, t5_data.rs:205-216) */
    uint32_t *d_tokenize_errors; /* device scalar (t5 tokenizer), 0 = ok; else bit 1: an item's ids
                                    exceeded their scratch, 2: id pool full, 3: long-item list full,
                                    4: a whitespace-free run longer than 256 KiB normalized (dropped);
                                    (gpt2 tokenizer) bit 0: more long pieces than their list holds
                                    (text_len / 64 + chunks + 1: the pieces past it get no ids);
                                    null for WordPiece.  Every call clears it first.  The gpt2 flag
                                    is reported here and checked by sdl_json_to_frames only: the
                                    host record path (sdl_batcher_push*) forwards the t5 flags alone. */
} sdl_device_rows;

int sdl_process_device(sdl_batcher *h, const uint8_t *d_text, uint64_t text_len,
                       const uint64_t *d_offsets, uint64_t n_records, uint64_t first_record,
                       void *stream, sdl_device_rows *out);

/* pack = 1: the 0 or 1 flush row of the handle's carry into row 0 of the device planes (*d_rows
 * says which), no host synchronisation; the carry is empty afterwards.  SDL_ERR_STATE when
 * pack = 0. */
int sdl_pack_flush_device(sdl_batcher *h, void *stream, sdl_device_rows *out);
/* pack = 1: the position_ids plane, device [rows_capacity, S], of the handle's last
 * sdl_process_device / sdl_pack_flush_device call; NULL when pack = 0 or before the first call. */
const int32_t *sdl_device_position_ids(sdl_batcher *h);

/* sdl_process_device for the multi-label task with Label::Multi indices per
 * record: record r's indices are d_labels[d_label_offsets[r] .. d_label_offsets[r+1])
 * (device memory, n_records+1 offsets).  SimpleBatcher::create_sync_batch
 * (simple_batcher.rs:35-43) + BertData MultiLabel (bert_data.rs:66-78). */
int sdl_process_device_labels(sdl_batcher *h, const uint8_t *d_text, uint64_t text_len,
                              const uint64_t *d_offsets, uint64_t n_records, const uint32_t *d_labels,
                              const uint64_t *d_label_offsets, uint64_t first_record, void *stream,
                              sdl_device_rows *out);

/* pair = 1: sdl_process_device_labels over n_pairs examples of two texts: A_r is text range 2r
 * and B_r range 2r+1 of the arena (d_offsets: 2 * n_pairs + 1 entries), so the tokenizer runs once
 * over 2 * n_pairs records.  *d_rows = n_pairs; d_record_rows has n_pairs entries, each 1;
 * d_tokens counts the ids of both sides before truncation; d_label_offsets has n_pairs + 1
 * entries; the label index of pair r is first_record + r. */
int sdl_process_device_pairs(sdl_batcher *h, const uint8_t *d_text, uint64_t text_len, const uint64_t *d_offsets,
                             uint64_t n_pairs, const uint32_t *d_labels, const uint64_t *d_label_offsets,
                             uint64_t first_record, void *stream, sdl_device_rows *out);
/* pair = 2..4: the pair labels, device int32 [rows_capacity], of the handle's last
 * sdl_process_device_pairs call (d_labels / d_label_offsets are ignored there; out->labels is the
 * MLM label plane); NULL when pair is 0 or 1, or before the first call. */
const int32_t *sdl_device_pair_labels(sdl_batcher *h);

/* ---- Provider step: the JsonText filter on the device ----------------------
 * SourceFilter::JsonText over inflated JSON lines (gzip_file_provider.rs:30-50
 * -> provider_util.rs:60-64: serde_json::from_str(line).unwrap(),
 * v["text"].as_str()): every '\n'-separated line whose value is an object with
 * a string member "text" (the last one if repeated) becomes one record, that
 * string unescaped to UTF-8, in a device text arena ready for
 * sdl_process_device.  Lines the reference's unwrap() panics on are skipped and
 * counted.  `d_jsonl` is device memory, 16-byte aligned and readable up to the
 * next multiple of 16 bytes past `len` (< 4 GiB).  The arena and offsets are
 * owned by the handle until the next call; the counts are copied to the host
 * (the call synchronises `stream`). */
typedef struct sdl_json_text {
    uint8_t *d_text;       /* device, 16-byte aligned: records back to back, 16 zero bytes after */
    uint64_t *d_offsets;   /* device [n_records + 1] */
    uint64_t n_records;
    uint64_t text_bytes;   /* = offsets[n_records] */
    uint64_t n_lines;      /* lines seen */
    uint64_t n_invalid;    /* lines the reference would panic on (skipped) */
} sdl_json_text;
int sdl_json_text_device(sdl_batcher *h, const uint8_t *d_jsonl, uint64_t len, void *stream, sdl_json_text *out);

/* ---- Provider step: gzip inflate on the device -----------------------------
 * Replaces the GzipDecoder under the provider's lines (gzip_file_provider.rs:
 * 13-28, async-compression 0.3.14 / flate2 1.0.24 / miniz_oxide 0.5.4): every
 * gzip member (RFC 1952; DEFLATE, RFC 1951) in `d_gz` is inflated by one wave,
 * members in parallel, and its CRC-32 and ISIZE are checked.  Member m is bytes
 * [d_member_offsets[m], d_member_offsets[m+1]) of d_gz (device, u64[n + 1]):
 * one file each (the reference decodes a file's first member), or the BGZF
 * blocks sdl_gzip_split_members finds in one file.  The outputs are written
 * back to back -- the JSON lines sdl_json_text_device takes as is.  d_gz is
 * device memory, 16-byte aligned, gz_len < 4 GiB, total output < 4 GiB.  A
 * corrupt member (where the reference's `next_line().await.unwrap()` panics)
 * makes the call return SDL_ERR_DATA with its index and reason; per-member
 * status codes stay readable in d_status.  The buffers are owned by the handle
 * until the next call; the call synchronises `stream` (the output size comes
 * from the members' trailers before anything is decoded). */
typedef struct sdl_inflated {
    uint8_t *d_out;             /* device, 16-byte aligned, 32 zero bytes after out_bytes */
    uint32_t *d_member_out;     /* device [n_members + 1]: member m's output is [d_member_out[m], [m+1]) */
    int32_t *d_status;          /* device [n_members]: 0 ok, else a GZ_* or ZS_* code */
    uint64_t out_bytes;
    uint64_t n_members;
    uint64_t n_bad;             /* members that failed */
} sdl_inflated;
int sdl_gzip_inflate_device(sdl_batcher *h, const uint8_t *d_gz, uint64_t gz_len, const uint64_t *d_member_offsets,
                            uint64_t n_members, void *stream, sdl_inflated *out);

/* The reference-exact variant (opt-in): every range [d_file_offsets[f],
 * d_file_offsets[f+1]) is one FILE, and only its first gzip member is inflated --
 * what async-compression's GzipDecoder with multiple_members off returns
 * (gzip_file_provider.rs:18, 64): `cat a.gz b.gz` yields a's lines, a BGZF file its
 * first block's.  The member's end is found on the device (the next offset where a
 * member header could start, else the file's end; a candidate inside the member's
 * own compressed data fails its decode and the next one is tried).  Output and
 * status as sdl_gzip_inflate_device, one member per file.  Limit: a first member
 * followed by bytes that hold no gzip header (trailing garbage) fails with
 * SDL_ERR_DATA (GZ_E_TRAIL) instead of being ignored. */
int sdl_gzip_inflate_first_device(sdl_batcher *h, const uint8_t *d_gz, uint64_t gz_len, const uint64_t *d_file_offsets,
                                  uint64_t n_files, void *stream, sdl_inflated *out);

/* Host only (no GPU): member byte ranges of one gzip file for
 * sdl_gzip_inflate_device.  BGZF files (every member carries the 'BC' extra
 * subfield with its size, as bgzip writes them) split into their members; any
 * other file is one member (async-compression's GzipDecoder reads the first
 * member of a file).  offsets gets *n_members + 1 entries (capacity `cap`
 * entries; SDL_ERR_CAPACITY with *n_members set when too small). */
int sdl_gzip_split_members(const uint8_t *gz, uint64_t len, uint64_t *offsets, uint64_t cap, uint64_t *n_members);

/* ---- Provider step: zstd frame decode on the device ------------------------
 * Replaces the ZstdDecoder under the provider's lines (zstd_file_provider.rs,
 * general_file_provider.rs:96-115: the .jsonl.zst datasets and the .json.zst cache):
 * every Zstandard frame (RFC 8878) in `d_zst` is decoded, all blocks of all frames
 * at once for the entropy stages.  Frame f is bytes [d_frame_offsets[f],
 * d_frame_offsets[f+1]) of d_zst (device, u64[n + 1]) -- what sdl_zstd_split_frames
 * returns for a file.  The output reuses sdl_inflated with frames in the place of
 * members: frame f's bytes are [d_member_out[f], d_member_out[f+1]) of d_out, back
 * to back (d_out 16-byte aligned, 32 zero bytes after); a skippable frame has zero
 * bytes and status 0.  d_zst is device memory, 16-byte aligned, zst_len < 4 GiB,
 * total output < 4 GiB.  A bad frame makes the call return SDL_ERR_DATA with its
 * index and reason in sdl_last_error(); per-frame ZS_* codes stay readable in
 * d_status, the good frames of the call are still decoded (a frame that failed
 * before its size was known has zero bytes, one that failed later -- offset
 * before the frame's start, checksum -- keeps its extent with undefined bytes).
 * A frame with a non-zero Dictionary_ID is refused: there are no dictionaries on
 * this path.  The XXH64 content checksum is verified where a frame carries one,
 * as libzstd does, unless SDL_ZSTD_NO_CHECKSUM is set in `flags`.  The buffers
 * are owned by the handle until the next call; the call synchronises `stream`.
 *
 * Reference semantics: async-compression's ZstdDecoder with multiple_members off
 * stops after the first frame (the generic decoder state machine it shares with
 * GzipDecoder), so the reference-exact call passes only the range of a file's
 * first non-skippable frame: offsets {o[k], o[k+1]} of sdl_zstd_split_frames. */
#define SDL_ZSTD_NO_CHECKSUM 1u
int sdl_zstd_inflate_device(sdl_batcher *h, const uint8_t *d_zst, uint64_t zst_len, const uint64_t *d_frame_offsets,
                            uint64_t n_frames, uint32_t flags, void *stream, sdl_inflated *out);

/* Host only (no GPU): the byte range of every frame of one .zst file, skippable
 * frames included, from the frame headers and the 3-byte block headers alone (no
 * entropy decode).  offsets gets *n_frames + 1 entries (capacity `cap` entries;
 * SDL_ERR_CAPACITY with *n_frames set when too small).  Bytes that are no frame
 * (bad magic, a reserved header bit, block type 3, a block over its maximum size,
 * truncation) return SDL_ERR_DATA. */
int sdl_zstd_split_frames(const uint8_t *zst, uint64_t len, uint64_t *offsets, uint64_t cap, uint64_t *n_frames);

/* ---- Transport step: batches as serde_pickle frames on the device ----------
 * Replaces serde_pickle::to_vec(&dataset, Default::default()) of each finished
 * DataSet (transport/zmq_transmit.rs:71, serde-pickle 1.1.1) that the Python
 * consumer reads with pickle.loads (python/external_dataset.py:52): the planes
 * of `rows` (from the last sdl_process_device[_labels] call of `h`) become one
 * frame per batch -- PROTO 3, the DataSet's fields in Serialize order
 * (bert_data.rs:106-145, gpt_data.rs:53-62, t5_data.rs:235-249), rows as lists
 * of BININT / BINFLOAT, STOP -- back to back in device memory.  Batches are the
 * n_rows / B full ones plus, when flush_partial and n_rows % B != 0, the
 * partial batch get_working_batch() would flush (its BertData `labels` list
 * holds the filled rows only).  `n_rows` is the value of *rows->d_rows (or
 * fewer rows).  The frames are owned by the handle until the next call; no
 * host synchronisation. */
typedef struct sdl_frames {
    uint8_t *d_frames;         /* device: frame f at f * frame_bytes */
    uint64_t n_frames;
    uint64_t frame_bytes;      /* bytes of every frame but the last */
    uint64_t last_frame_bytes; /* bytes of the last frame */
    uint64_t total_bytes;
} sdl_frames;
int sdl_pickle_frames_device(sdl_batcher *h, const sdl_device_rows *rows, uint64_t n_rows, int flush_partial,
                             void *stream, sdl_frames *out);

/* ---- End to end, host to host: JSON lines in, socket bytes out -------------
 * The reference's Provider -> Batcher -> Transport path for a buffer of
 * inflated JSON lines in host memory (gzip_file_provider.rs:30-50 ->
 * provider_util.rs:60-64 -> create_batch, batcher.rs:33-77 -> zmq_transmit.rs:71):
 * JsonText, tokenize + mask and serde_pickle frames on the device, in chunks of
 * about chunk_bytes (cut at line ends; 0 = 8 MiB) on three streams, so one
 * chunk's frames copy out while the next is copied in and computed.  Every
 * frame is handed to sink(user, frame, bytes) in order (sink may be NULL: the
 * frames still reach host memory); a non-zero return stops the call.  The
 * frames are those of the whole buffer in one sdl_json_text_device +
 * sdl_process_device + sdl_pickle_frames_device call: every full batch (rows
 * short of a batch carry into the next chunk), then the partial batch when
 * flush_partial.  Tasks mlm, clm and span (JSON lines carry no labels). */
typedef int (*sdl_frame_sink)(void *user, const uint8_t *frame, uint64_t bytes);
typedef struct sdl_json_frames_stats {
    uint64_t n_lines, n_invalid, n_records, text_bytes, n_rows, n_frames, frame_bytes, n_chunks;
    double seconds;  /* wall time of the call */
    double host_wait[4];  /* host time in: JsonText (its sizing syncs), tokenize + mask to the row count,
                             frames + copy-out issue, waiting for earlier copies out (delivery) */
} sdl_json_frames_stats;
int sdl_json_to_frames(sdl_batcher *h, const uint8_t *jsonl, uint64_t len, uint64_t chunk_bytes, int flush_partial,
                       sdl_frame_sink sink, void *user, sdl_json_frames_stats *stats);

/* ---- Several GPUs, one record stream ---------------------------------------
 * Records are independent (gen_batcher.rs:69-94 touches only the record's ids and
 * the row cursor), so N Batchers on N contiguous record ranges emit what N
 * reference Batchers (runner_simple.rs:68-112 runs one) would on those shards;
 * masks are keyed by the global record index, so every row equals the row one
 * handle would give over the whole stream.  No collective is involved.
 *
 * Host only: cut records [0, n_records) into n_shards contiguous ranges of about
 * equal bytes -- bounds[k] = the first record starting at or past
 * offsets[0] + k * (offsets[n_records] - offsets[0]) / n_shards, bounds[0] = 0,
 * bounds[n_shards] = n_records (n_shards + 1 entries; a range may be empty). */
int sdl_shard_records(const uint64_t *offsets, uint64_t n_records, uint32_t n_shards, uint64_t *bounds);

typedef struct sdl_multi sdl_multi;
/* One handle (own HIP stream) per entry of devices[0 .. n_devices), cfg->device
 * ignored; a device may repeat.  cfg->first_record is the global index of the
 * first record of the first push. */
int sdl_multi_create(const sdl_config *cfg, const char *tokenizer_path, const char *data_dir,
                     const int32_t *devices, uint32_t n_devices, sdl_multi **out);
void sdl_multi_destroy(sdl_multi *m);
/* sdl_batcher_push_many over one record stream: cut by sdl_shard_records into
 * one shard per handle, every shard pushed into its handle on its own host thread
 * (after hipSetDevice of its device; the calling thread runs shard 0 and is left on
 * devices[0]), shard k's records keyed from the global index of its first record.
 * n_emitted[k] (n_devices entries, may be NULL) = batches shard k queued; pop them
 * with sdl_batcher_next / sdl_batcher_flush on sdl_multi_handle(m, k).  The global
 * record index continues across calls.  When a shard fails, the shards that
 * succeeded have queued their batches: n_emitted is written for every shard either
 * way (0 for a failed one), and the multi handle is poisoned -- later pushes return
 * SDL_ERR_STATE -- since re-pushing the records would duplicate the committed
 * shards' rows. */
int sdl_multi_push_many(sdl_multi *m, const uint8_t *arena, const uint64_t *offsets, size_t n_records,
                        const uint32_t *labels, const uint64_t *label_offsets, size_t *n_emitted);
/* Shard k's handle (also for sdl_process_device on a device-resident shard with
 * first_record = its bound); NULL when k >= n_devices. */
sdl_batcher *sdl_multi_handle(sdl_multi *m, uint32_t k);

/* Copies `bytes` from device memory (e.g. sdl_device_rows planes) to host
 * memory with the handle's HIP runtime, ordered after the handle's work on
 * `stream` (NULL = the handle's stream); returns when the copy is complete. */
int sdl_device_to_host(sdl_batcher *h, void *dst, const void *src, size_t bytes, void *stream);

/* Per-stage device time (ms) of the last sdl_process_device or sdl_zstd_inflate_device
 * call, measured with hipEvents on the stream the kernels ran on, when enabled. */
int sdl_set_profiling(sdl_batcher *h, int enable);
int sdl_stage_times(sdl_batcher *h, const char **names, float *ms, int cap);

/* Loads and checks a tokenizer on the host only (no GPU needed): what
 * sdl_batcher_create would accept.  kind: 0 WordPiece, 1 byte-level BPE,
 * 2 Unigram (t5). */
typedef struct sdl_tokenizer_info {
    int32_t kind;
    int32_t vocab_size;
    int32_t n_added;            /* added tokens matched on the raw text */
    int32_t unk_id;
    int32_t eos_id;             /* </s> / <|endoftext|> (TokenizerInfo.eos), -1 if none */
    int32_t max_piece_bytes;
    uint64_t word_table_entries; /* device word-table / hash entries */
    int32_t normalizer_flags;   /* WordPiece BertNormalizer: bit 0 keeps case (lowercase=false),
                                 * bit 1 keeps accents (strip_accents=false); 0 otherwise */
    int32_t reserved[5];
} sdl_tokenizer_info;
int sdl_tokenizer_info_get(const char *tokenizer_path, const char *data_dir, sdl_tokenizer_info *out);

/* Last error message of the calling thread. */
const char *sdl_last_error(void);
int sdl_abi_version(void);
/* sha256 (hex) of the sources, headers and flags this library was built from
 * (streaming_data_loader_amd/build.py source_hash): proves which build ran. */
const char *sdl_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* SDL_BATCHER_H */
