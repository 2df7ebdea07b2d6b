"""GPU parity of MLM sentence pairs (sdl_config.pair 2..4, DESIGN.md §3 "Sentence pairs"): one
[CLS] A [SEP] B [SEP] row per example with a BERT masking policy applied and a pair label drawn
(as given, next-sentence, sentence-order).

Every comparison is exact, plane for plane -- input_ids, attention_mask, token_type_ids, labels, the
pair labels, and the rows up to the next multiple of B that nobody filled -- against
pair_mlm_model.py, which test_pair_mlm_model.py ties to csrc/pair_draw.hpp, to tokenizers'
encode(first, second) and to the masking model.  The ids of each side come from the C oracle's
WordPiece.  Covered: every mode x policy at S in {8, 9, 16, 17, 128} with side lengths swept around
M/2, M and 3M, empty sides and a B much longer than its A; every MR of the kernel; a call of several
hundred KiB past the small-call threshold, its records straddling chunk edges and a source B in a
far chunk, then a short call on the same handle; first_record across 2^32 and a second seed; calls
of one and two pairs; the host calls, their cadence and the batch's pair labels; the transport
frames' fifth key; and every new refusal by status code and a word of its message."""
import ctypes
import pickle
import random

import numpy as np
import pytest

import mlm_policy_model as P
import oracle_lib
import pair_mlm_model as M
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher, arena_from_pairs

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED, ERR_STATE = -1, -4, -6
MODES = (native.SDL_PAIR_MLM, native.SDL_PAIR_MLM_NSP, native.SDL_PAIR_MLM_SOP)
SEED = 20240229
NAMES = ("input_ids", "attention_mask", "token_type_ids", "labels")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def enc(oracle_tok):
    e = oracle_lib.Encoder("bert", oracle_tok)
    assert tuple(e.tok.encode("")) == (101, 102) and P.proxy_vocab()[2:] == (101, 102)
    return e


def wp_ids(tok, text):
    return tok.encode(text)[1:-1]  # (the oracle's encode adds the template's [CLS] and [SEP])


def words_text(rng, n_ids, tok):
    """A text of exactly n_ids ids: common words (one piece each) and random letter runs (several
    pieces, so that whole-word units exist), trimmed word by word."""
    words, total = [], 0
    while total < n_ids:
        w = P.random_word(rng) if rng.random() < 0.4 else rng.choice(P.COMMON)
        k = len(wp_ids(tok, w))
        if total + k > n_ids:
            w = rng.choice(P.COMMON)
            k = len(wp_ids(tok, w))
            assert k == 1
        words.append(w)
        total += k
    return " ".join(words)


def swept_lengths(S, n=37):
    """n (n_a, n_b) in ids: around M/2, M and 3M on either side, an empty A, an empty B, both empty,
    and a B much longer than its A (a foreign B then changes k_a)."""
    Mx = S - 3
    L = sorted({max(0, x) for x in (0, 1, 2, Mx // 2 - 1, Mx // 2, Mx // 2 + 1, Mx - 1, Mx, Mx + 1, 3 * Mx)})
    lens = [(0, 0), (0, Mx), (Mx, 0), (1, 3 * Mx), (2, 3 * Mx + 5), (3 * Mx, 1), (Mx // 2, Mx // 2), (Mx, Mx)]
    rng = random.Random(S)
    while len(lens) < n:
        lens.append((rng.choice(L), rng.choice(L)))
    return lens


@pytest.fixture(scope="module")
def swept(enc):
    """Per S: the 37 pairs of texts and their ids (computed once, shared by the modes and policies)."""
    out = {}
    for S in (8, 9, 16, 17, 128):
        rng = random.Random(1000 + S)
        texts = [(words_text(rng, a, enc.tok), words_text(rng, b, enc.tok)) for a, b in swept_lengths(S)]
        ids = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in texts]
        assert [(len(a), len(b)) for a, b in ids] == swept_lengths(S)
        out[S] = (texts, ids)
    return out


def to_device(torch, pairs):
    arena, offs = arena_from_pairs(pairs)
    pad = np.zeros(arena.size + 16, np.uint8)
    pad[:arena.size] = arena
    return torch.from_numpy(pad).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), int(arena.size)


def run_pairs(torch, db, pairs, first_record=0):
    ta, to, n = to_device(torch, pairs)
    res = db.process_pairs(ta.data_ptr(), n, to.data_ptr(), len(pairs), first_record=first_record)
    torch.cuda.synchronize()
    return res, n


def assert_call(res, want, n, Bsz):
    """The call's planes and pair labels over every row up to the next multiple of B."""
    G = -(-n // Bsz) * Bsz
    assert res.rows() == n and res.r.rows_capacity >= G and res.r.label_width == want["planes"].shape[2]
    assert want["planes"].shape[1] == G
    got = res.planes(G)
    for name, g, w in zip(NAMES, got, want["planes"]):
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, f"{name}: {bad.size} rows differ, first {bad[:5]}: {g[bad[0]]} != {w[bad[0]]}"
    np.testing.assert_array_equal(res.pair_labels(G), want["pair_labels"])
    np.testing.assert_array_equal(res.record_rows(), np.ones(n, np.uint32))


def make(mode, policy, S, Bsz, seed=SEED, mask_length=None, per_mille=250, **kw):
    return DeviceBatcher(task=native.SDL_TASK_MLM, batch_size=Bsz, sequence_length=S, pair=mode, mask_policy=policy,
                         mask_per_mille=per_mille, seed=seed,
                         mask_length=max(1, S // 5) if mask_length is None else mask_length, **kw)


def model(ids, S, mode, policy, Bsz, seed=SEED, first_record=0, mask_length=None, per_mille=250):
    return M.rows(ids, S, mode, policy, seed, first_record, max(1, S // 5) if mask_length is None else mask_length,
                  per_mille, B=Bsz)


# ---- 1. main parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S", [8, 9, 16, 17, 128])
def test_modes_and_policies_match_the_model(torch, native_lib, swept, S, mode, policy):
    texts, ids = swept[S]
    Bsz, n = 8, len(texts)
    assert n == 37 and n % Bsz  # a partial last batch
    db = make(mode, policy, S, Bsz)
    res, _ = run_pairs(torch, db, texts, first_record=5)
    want = model(ids, S, mode, policy, Bsz, first_record=5)
    assert_call(res, want, n, Bsz)
    assert res.tokens() == sum(len(a) + len(b) for a, b in ids)
    lab = want["pair_labels"][:n]
    assert (lab == 0).all() if mode == native.SDL_PAIR_MLM else 0 < lab.sum() < n
    if S >= 16:
        assert any(i["sel"] for i in want["infos"]) and (want["planes"][0] == 103).any()
    if mode == native.SDL_PAIR_MLM:  # both empty: [CLS] [SEP] [SEP] and no pick
        assert want["planes"][0, 0, :4].tolist() == [101, 102, 102, 0] and (want["planes"][3, 0] == -100).all()
    if mode == native.SDL_PAIR_MLM_NSP:  # a foreign, much longer B changed some row's k_a
        own = M.rows(ids, S, native.SDL_PAIR_MLM, policy, SEED, 5, max(1, S // 5), 250, B=Bsz)["planes"]
        a_len = lambda pl: (np.cumsum(pl[2], axis=1) == 0).sum(axis=1)  # noqa: E731  (positions before the first type 1)
        assert (a_len(own)[:n] != a_len(want["planes"])[:n]).any()
    db.close()


# ---- 2. every MR ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [256, 260, 520, 1028, 2048])
def test_every_row_width_of_the_kernel(torch, native_lib, enc, S):
    Mx = S - 3
    lens = [(Mx // 2, Mx // 2 + 1), (Mx, Mx), (3 * Mx, 7), (5, 3 * Mx), (0, 2 * Mx), (Mx - 1, 1), (0, 0), (40, 60),
            (Mx // 2 - 1, Mx // 2 - 1), (Mx // 3, 2 * Mx), (Mx + 1, 0), (300, 200)]
    rng = random.Random(S)
    texts = [(words_text(rng, a, enc.tok), words_text(rng, b, enc.tok)) for a, b in lens]
    ids = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in texts]
    db = make(native.SDL_PAIR_MLM_NSP, 2, S, 8)
    res, _ = run_pairs(torch, db, texts)
    want = model(ids, S, native.SDL_PAIR_MLM_NSP, 2, 8)
    assert_call(res, want, len(texts), 8)
    # picks in the last round of positions, and words of several pieces taken whole
    assert any(i["sel"] and i["sel"][-1] >= 256 * ((S - 1) // 256) for i in want["infos"])
    assert any(len(u) > 1 and u[0] in i["sel"] for i in want["infos"] for u in i["units"])
    db.close()


# ---- 3. chunk lists ------------------------------------------------------------------------------
def random_text(rng, lengths=(0, 1, 5, 40, 200, 700, 1500, 2000)):
    alphabet = "abcdefghij klmnop,.;!? ÄéßİＡ中文​\t\n"
    return "".join(rng.choice(alphabet) for _ in range(rng.choice(lengths)))


def test_long_call_then_short_call_on_one_handle(torch, native_lib, enc):
    rng = random.Random(18)
    pairs = [(random_text(rng), random_text(rng)) for _ in range(260)]
    ids = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in pairs]
    S, Bsz, mode = 128, 64, native.SDL_PAIR_MLM_NSP
    db = make(mode, 2, S, Bsz)
    res, nbytes = run_pairs(torch, db, pairs, first_record=1000)
    assert nbytes > 200 << 10  # past SMALL_CHUNKS x 1 KiB chunks
    offs = arena_from_pairs(pairs)[1].astype(np.int64)
    assert sum(1 for q in range(len(offs) - 1) if offs[q] // 1024 != (offs[q + 1] - 1) // 1024 and offs[q + 1] > offs[q]) > 50
    # a source B in a far chunk: a random row whose B starts over 100 chunks away from its A
    far = 0
    for r in range(len(pairs)):
        f, s, lab = M.draw(SEED, 1000 + r, r, len(pairs), mode)
        far += bool(lab and abs(int(offs[s]) - int(offs[f])) > 100 * 1024 and len(ids[(s - 1) // 2][1]) > 0)
    assert far > 10
    assert_call(res, model(ids, S, mode, 2, Bsz, first_record=1000), len(pairs), Bsz)
    # a short call on the same handle: nothing of the long one shows
    short = [("one two three", "four"), ("", "five six"), ("seven", "")]
    sids = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in short]
    res2, _ = run_pairs(torch, db, short, first_record=7)
    assert_call(res2, model(sids, S, mode, 2, Bsz, first_record=7), 3, Bsz)
    db.close()


# ---- 4. first_record and the seed ----------------------------------------------------------------
def test_first_record_across_the_high_word_and_a_second_seed(torch, native_lib, swept):
    texts, ids = swept[17]
    S, Bsz, mode, first = 17, 8, native.SDL_PAIR_MLM_NSP, 2**32 - 3
    db = make(mode, 1, S, Bsz)
    res, _ = run_pairs(torch, db, texts, first_record=first)
    want = model(ids, S, mode, 1, Bsz, first_record=first)
    assert_call(res, want, len(texts), Bsz)
    got = res.planes(len(texts)) + (res.pair_labels(len(texts)),)
    at0 = model(ids, S, mode, 1, Bsz, first_record=0)
    assert (at0["planes"][3] != want["planes"][3]).any() and (at0["pair_labels"] != want["pair_labels"]).any()
    db.close()
    db2 = make(mode, 1, S, Bsz, seed=SEED + 1)
    res2, _ = run_pairs(torch, db2, texts, first_record=first)
    assert_call(res2, model(ids, S, mode, 1, Bsz, seed=SEED + 1, first_record=first), len(texts), Bsz)
    got2 = res2.planes(len(texts)) + (res2.pair_labels(len(texts)),)
    assert (got[0] != got2[0]).any() and (got[3] != got2[3]).any() and (got[4] != got2[4]).any()
    db2.close()


# ---- 5. tiny calls -------------------------------------------------------------------------------
def test_calls_of_one_and_two_pairs(torch, native_lib, enc):
    S, Bsz, mode = 16, 4, native.SDL_PAIR_MLM_NSP
    db = make(mode, 1, S, Bsz)
    one = [("the of and to in a", "is that for it as was with be")]
    oid = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in one]
    for first in range(6):  # never random: label 0, its own B, whatever the coin says
        res, _ = run_pairs(torch, db, one, first_record=first)
        want = model(oid, S, mode, 1, Bsz, first_record=first)
        assert_call(res, want, 1, Bsz)
        assert res.pair_labels(1).tolist() == [0] and (res.planes(1)[2][0] == want["planes"][2, 0]).all()
    assert any(M.draw_words(SEED, first)[0] >= M.HALF for first in range(6))
    two = one + [("by on not he this", "are or his")]
    tid = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in two]
    seen = set()
    for first in range(0, 12, 2):
        res, _ = run_pairs(torch, db, two, first_record=first)
        assert_call(res, model(tid, S, mode, 1, Bsz, first_record=first), 2, Bsz)
        seen |= set(enumerate(res.pair_labels(2).tolist()))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # a call of no pairs: no rows
    ta, to, _ = to_device(torch, one)
    res0 = db.process_pairs(ta.data_ptr(), 0, to.data_ptr(), 0)
    torch.cuda.synchronize()
    assert res0.rows() == 0
    db.close()


# ---- 6. host path --------------------------------------------------------------------------------
def host_pairs(n, seed):
    rng = random.Random(seed)
    L = (0, 1, 5, 40, 200, 700)
    return [(random_text(rng, L), random_text(rng, L)) for _ in range(n)]


def make_gen(mode, policy, Bsz, S, seed=SEED):
    return B.GenTokenizer(B.ModelType.Bert, B.BatchConfig(Bsz, S), B.Mask(max(1, S // 5), 103, policy, 250, pair=mode),
                          B.TokenizerConfig(), seed=seed)


def assert_batches(got, calls, Bsz, key):
    """`calls`: the model's planes of each call, row-concatenated in stream order."""
    planes = np.concatenate([c["planes"] for c in calls], axis=1)
    plab = np.concatenate([c["pair_labels"] for c in calls])
    n = planes.shape[1]
    assert [ds.rows for ds in got] == [min(Bsz, n - b0) for b0 in range(0, n, Bsz)]
    for i, ds in enumerate(got):
        sl = slice(i * Bsz, i * Bsz + ds.rows)
        r = ds.rows
        for name, g, w in zip(NAMES, (ds.input_ids, ds.attention_mask, ds.token_type_ids, ds.labels), planes):
            np.testing.assert_array_equal(g[:r], w[sl], err_msg=f"batch {i} {name}")
        np.testing.assert_array_equal(ds.pair_labels[:r], plab[sl], err_msg=f"batch {i}")
        # the rows nobody filled
        assert (ds.input_ids[r:] == 0).all() and (ds.attention_mask[r:] == 1).all() and (ds.token_type_ids[r:] == 0).all()
        assert (ds.labels[r:] == -100).all() and (ds.pair_labels[r:] == -100).all() and ds.pair_labels.shape == (Bsz,)
        d = ds.to_dict()
        assert list(d) == list(NAMES) + [key]
        np.testing.assert_array_equal(d[key], plab[sl])


def test_host_path_bulk_cadence_and_flush(native_lib, enc):
    Bsz, S, mode, policy = 16, 32, native.SDL_PAIR_MLM_NSP, 2
    pairs = host_pairs(70, seed=9)
    ids = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in pairs]
    # two calls that split a batch: each is one call for the draw, keyed from the pairs before it
    gt = make_gen(mode, policy, Bsz, S)
    got = gt.create_sync_batches_pairs(pairs[:25])
    assert len(got) == 1
    got += gt.create_sync_batches_pairs(pairs[25:])
    assert len(got) == 70 // Bsz
    got.append(gt.get_working_batch())
    kw = dict(mask_length=max(1, S // 5), per_mille=250)
    calls = [M.rows(ids[:25], S, mode, policy, SEED, 0, **kw), M.rows(ids[25:], S, mode, policy, SEED, 25, **kw)]
    assert_batches(got, calls, Bsz, "next_sentence_label")
    assert any(ds.pair_labels[:ds.rows].any() for ds in got)
    # not the rows of one call over all 70 (the draw depends on the cut into calls)
    whole = M.rows(ids, S, mode, policy, SEED, 0, **kw)
    assert (whole["planes"][0] != np.concatenate([c["planes"][0] for c in calls], axis=0)).any()
    # push_arena(..., pairs=True) is the same call
    gt2 = make_gen(mode, policy, Bsz, S)
    arena, offs = arena_from_pairs(pairs[:25])
    got2 = gt2.push_arena(arena, offs, pairs=True) + [gt2.get_working_batch()]
    assert_batches(got2, calls[:1], Bsz, "next_sentence_label")


@pytest.mark.parametrize("mode", [native.SDL_PAIR_MLM, native.SDL_PAIR_MLM_SOP])
def test_host_path_one_pair_a_call(native_lib, enc, mode):
    Bsz, S, policy = 4, 17, 1
    pairs = host_pairs(10, seed=mode)
    ids = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in pairs]
    gt = make_gen(mode, policy, Bsz, S)
    got = []
    for i, (a, b) in enumerate(pairs):
        ds = gt.create_sync_batch_pair(a, b)
        assert (ds is not None) == ((i + 1) % Bsz == 0), i
        if ds is not None:
            got.append(ds)
    got.append(gt.get_working_batch())
    calls = [M.rows(ids[i:i + 1], S, mode, policy, SEED, i, mask_length=max(1, S // 5), per_mille=250)
             for i in range(len(pairs))]
    key = "sentence_order_label" if mode == native.SDL_PAIR_MLM_SOP else "next_sentence_label"
    assert_batches(got, calls, Bsz, key)
    labs = np.concatenate([c["pair_labels"] for c in calls])
    assert (labs == 0).all() if mode == native.SDL_PAIR_MLM else 0 < labs.sum() < len(pairs)


# ---- 7. frames -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_frames_carry_the_pair_labels(torch, native_lib, enc, mode):
    Bsz, S, policy = 8, 17, 1
    pairs = host_pairs(21, seed=4)
    ids = [(wp_ids(enc.tok, a), wp_ids(enc.tok, b)) for a, b in pairs]
    db = make(mode, policy, S, Bsz)
    res, _ = run_pairs(torch, db, pairs)
    want = model(ids, S, mode, policy, Bsz)
    frames = db.pickle_frames(res, len(pairs), flush_partial=True).frames()
    assert len(frames) == 3
    key = "sentence_order_label" if mode == native.SDL_PAIR_MLM_SOP else "next_sentence_label"
    for i, f in enumerate(frames):
        d = pickle.loads(f)
        r = min(Bsz, len(pairs) - i * Bsz)
        sl = slice(i * Bsz, (i + 1) * Bsz)
        assert list(d) == list(NAMES) + [key]
        for k, name in enumerate(NAMES[:3]):
            assert d[name] == want["planes"][k][sl].tolist(), (i, name)
        assert d["labels"] == want["planes"][3][i * Bsz:i * Bsz + r].tolist()
        assert d[key] == want["pair_labels"][i * Bsz:i * Bsz + r].tolist() and len(d[key]) == r
        # the four mlm keys are the bytes of an unpaired mlm frame of the same planes
        ref = oracle_lib.pickle_dataset("mlm", Bsz, S, S, r, *[np.ascontiguousarray(want["planes"][k][sl]) for k in range(4)])
        assert f[:len(ref) - 2] == ref[:-2]
    # full frames only
    assert len(db.pickle_frames(res, len(pairs), flush_partial=False).frames()) == 2
    db.close()


# ---- 8. refusals ---------------------------------------------------------------------------------
def create_rc(native_lib, task, pair, tokenizer=native.BERT_PROXY_TOKENIZER, S=16, mask_policy=1, rng_mode=0):
    c = native.default_config(task)
    c.batch_size, c.sequence_length, c.pair = 4, S, pair
    c.mask_length = min(c.mask_length, 2)
    c.mask_policy, c.rng_mode = mask_policy, rng_mode
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), tokenizer.encode(), native.DATA_DIR.encode(), ctypes.byref(h))
    msg = native_lib.sdl_last_error().decode() if rc else ""
    if h.value:
        native_lib.sdl_batcher_destroy(h)
    return rc, msg


def test_create_refusals(torch, native_lib):
    for mode in MODES:
        for task in (native.SDL_TASK_CLM, native.SDL_TASK_SPAN, native.SDL_TASK_MULTI_LABEL,
                     native.SDL_TASK_SINGLE_CLASS):
            rc, msg = create_rc(native_lib, task, mode, mask_policy=0)
            assert rc == ERR_ARG and "pair" in msg and "MLM" in msg
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, mask_policy=0)
        assert rc == ERR_UNSUPPORTED and "pair" in msg and "mask_policy 0" in msg
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, rng_mode=1)
        assert rc == ERR_UNSUPPORTED and "pair" in msg and "rng_mode" in msg
        for tokenizer in (native.GPT2_PROXY_TOKENIZER, native.T5_PROXY_TOKENIZER):
            for policy in (1, 2):
                rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, tokenizer, mask_policy=policy)
                assert rc == ERR_UNSUPPORTED and "pair" in msg and "BPE or Unigram" in msg
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, S=2)
        assert rc == ERR_ARG and "pair" in msg and "sequence_length >= 3" in msg
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, S=2049)
        assert rc == ERR_ARG and "pair" in msg and "2048" in msg
        assert create_rc(native_lib, native.SDL_TASK_MLM, mode, S=3)[0] == 0
        assert create_rc(native_lib, native.SDL_TASK_MLM, mode, S=2048, mask_policy=2)[0] == 0
        c = native.default_config(native.SDL_TASK_MLM)
        c.batch_size, c.sequence_length, c.pair, c.mask_policy = 4, 16, mode, 1
        m = ctypes.c_void_p()
        devs = (ctypes.c_int32 * 1)(0)
        assert native_lib.sdl_multi_create(ctypes.byref(c), native.BERT_PROXY_TOKENIZER.encode(),
                                           native.DATA_DIR.encode(), devs, 1, ctypes.byref(m)) == ERR_UNSUPPORTED
        assert "pair" in native_lib.sdl_last_error().decode() and not m.value
    # the earlier refusals stand
    rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, 1)
    assert rc == ERR_UNSUPPORTED and "mlm, clm or span" in msg
    for bad in (5, 7, -1):
        assert create_rc(native_lib, native.SDL_TASK_MLM, bad)[0] == ERR_ARG


def test_call_refusals_and_accessors(torch, native_lib):
    L, vp = native_lib, ctypes.c_void_p
    ta, to, n = to_device(torch, [("a b", "c")])
    rows, batch, emitted = native.DeviceRows(), native.Batch(), ctypes.c_size_t()
    nsp = make(native.SDL_PAIR_MLM_NSP, 1, 16, 4)
    sop = make(native.SDL_PAIR_MLM_SOP, 1, 16, 4)
    rows1 = DeviceBatcher(task=native.SDL_TASK_SINGLE_CLASS, batch_size=4, sequence_length=16, pair=True)
    plain = DeviceBatcher(task=native.SDL_TASK_MLM, batch_size=4, sequence_length=16, mask_policy=1, mask_length=2)
    # one pair a call has nobody to draw from
    assert L.sdl_batcher_push_pair(nsp._h, b"a", 1, b"b", 1, None, 0, ctypes.byref(batch)) == ERR_UNSUPPORTED
    assert "pair = 3" in L.sdl_last_error().decode()
    assert L.sdl_batcher_push_pair(sop._h, b"a", 1, b"b", 1, None, 0, ctypes.byref(batch)) == 0
    # the unpaired calls on a pair-mlm handle, and the JSON path
    offs = (ctypes.c_uint64 * 3)(0, 1, 2)
    assert L.sdl_process_device(nsp._h, vp(ta.data_ptr()), n, vp(to.data_ptr()), 2, 0, None, ctypes.byref(rows)) == ERR_STATE
    assert L.sdl_batcher_push(nsp._h, b"ab", 2, None, 0, ctypes.byref(batch)) == ERR_STATE
    assert L.sdl_batcher_push_many(nsp._h, b"ab", offs, 2, None, None, ctypes.byref(emitted)) == ERR_STATE
    stats = native.JsonFramesStats()
    line = b'{"text": "a"}\n'
    for h in (nsp, sop):
        assert L.sdl_json_to_frames(h._h, line, len(line), 0, 1, ctypes.cast(None, native.FRAME_SINK), None,
                                    ctypes.byref(stats)) == ERR_UNSUPPORTED
        assert "pair" in L.sdl_last_error().decode()
    # the pair calls on an unpaired mlm handle
    assert L.sdl_process_device_pairs(plain._h, vp(ta.data_ptr()), n, vp(to.data_ptr()), 1, None, None, 0, None,
                                      ctypes.byref(rows)) == ERR_STATE
    # the accessors: NULL off pair 2..4 and before the first call
    assert not L.sdl_device_pair_labels(plain._h) and not L.sdl_device_pair_labels(rows1._h)
    assert not L.sdl_device_pair_labels(nsp._h)
    res = nsp.process_pairs(ta.data_ptr(), n, to.data_ptr(), 1)
    torch.cuda.synchronize()
    assert L.sdl_device_pair_labels(nsp._h) and res.pair_labels(4).tolist() == [0, -100, -100, -100]
    tl = torch.tensor([1], dtype=torch.int32).cuda()
    tlo = torch.tensor([0, 1], dtype=torch.int64).cuda()
    r1 = rows1.process_pairs(ta.data_ptr(), n, to.data_ptr(), 1, tl.data_ptr(), tlo.data_ptr())
    torch.cuda.synchronize()
    assert r1.pair_labels() is None and not L.sdl_device_pair_labels(rows1._h)
    gt = B.GenTokenizer(B.ModelType.Bert, B.BatchConfig(1, 16), B.Mask(2, 103, 1), B.TokenizerConfig())
    ds = gt.create_sync_batch("x " * 80)
    assert ds is not None and ds.pair_labels is None and list(ds.to_dict()) == list(NAMES)
    for h in (nsp, sop, rows1, plain):
        h.close()
