"""The sentence-pair contract (pair_model.py; sdl_config.pair = 1) against its authority (CPU):
tokenizers' encode(a, b) on the bert proxy tokenizer.json -- BertProcessing, longest_first
truncation to S, padding to S -- in input_ids, token_type_ids and attention_mask.

Every (n_a, n_b) in 0..2S for S in {8, 9, 16, 17} with texts built from a word the proxy
vocabulary holds as one piece, then a few hundred random texts in test_single_class.py's
alphabet.  Also: the ctypes mirror's `pair` word is the last word of sdl_config, and the Python
mirror's helpers lay pairs out as the C ABI takes them."""
import ctypes
import random

import numpy as np
import pytest
import tokenizers

import pair_model
from streaming_data_loader_amd import native

WORD = "the"  # one piece of the proxy vocabulary (asserted below)


@pytest.fixture(scope="module")
def plain():
    return tokenizers.Tokenizer.from_file(native.BERT_PROXY_TOKENIZER)


def library_rows(S, pairs):
    tk = tokenizers.Tokenizer.from_file(native.BERT_PROXY_TOKENIZER)
    tk.enable_truncation(max_length=S, strategy="longest_first")
    tk.enable_padding(length=S)
    out = []
    for a, b in pairs:
        e = tk.encode(a, b)
        out.append((e.ids, e.type_ids, e.attention_mask))
    return out


def specials(plain):
    return plain.token_to_id("[CLS]"), plain.token_to_id("[SEP]")


def check(plain, S, pairs):
    cls, sep = specials(plain)
    want = library_rows(S, pairs)
    for (a, b), (ids, tt, am) in zip(pairs, want):
        ia = plain.encode(a, add_special_tokens=False).ids
        ib = plain.encode(b, add_special_tokens=False).ids
        g_ids, g_tt, g_am = pair_model.pair_row(ia, ib, S, cls, sep)
        key = (S, len(ia), len(ib))
        assert len(ids) == S, key
        assert g_ids.tolist() == ids, key
        assert g_tt.tolist() == tt, key
        assert g_am.tolist() == am, key


@pytest.mark.parametrize("S", [8, 9, 16, 17])
def test_every_length_pair_matches_tokenizers(plain, S):
    for n in (0, 1, 5, 2 * S):
        assert len(plain.encode(" ".join([WORD] * n), add_special_tokens=False).ids) == n
    texts = [" ".join([WORD] * n) for n in range(2 * S + 1)]
    check(plain, S, [(a, b) for a in texts for b in texts])


def random_text(rng):
    alphabet = "abcdefghij klmnop,.;!? ÄéßİＡ中文​\t\n"
    L = rng.choice([0, 1, 5, 12, 40, 90])
    return "".join(rng.choice(alphabet) for _ in range(L))


@pytest.mark.parametrize("S", [8, 9, 16, 17, 32])
def test_random_texts_match_tokenizers(plain, S):
    rng = random.Random(1000 + S)
    check(plain, S, [(random_text(rng), random_text(rng)) for _ in range(300)])


def test_kept_lengths_properties():
    for S in (3, 4, 8, 9, 16, 17, 128):
        M = S - 3
        for na in range(0, 2 * S + 2):
            for nb in range(0, 2 * S + 2):
                ka, kb = pair_model.kept_lengths(na, nb, S)
                assert 0 <= ka <= na and 0 <= kb <= nb
                assert ka + kb == min(na + nb, M), (S, na, nb)
                if na == nb and na + nb > M:  # a tie: B gets the odd id
                    assert (ka, kb) == (M // 2, M // 2 + M % 2)


def test_config_pair_word(native_lib):
    """`pair` is the last word of sdl_config (the header's former reserved tail); a default
    config leaves it 0."""
    assert native.Config.pair.offset == 92 and native.Config.pair.size == 4
    assert ctypes.sizeof(native.Config) == 96
    for task in (native.SDL_TASK_MLM, native.SDL_TASK_SINGLE_CLASS, native.SDL_TASK_MULTI_LABEL):
        c = native.default_config(task)
        assert c.pair == 0
        c.pair = 1
        assert list(c.reserved) == [0, 0, 0, 1]


def test_pair_arena_layout():
    from streaming_data_loader_amd.device import arena_from_pairs, arena_from_texts
    pairs = [("a b", "c"), ("", "héllo"), ("x" * 40, ""), ("", "")]
    arena, offs = arena_from_pairs(pairs)
    flat = [t for p in pairs for t in p]
    a2, o2 = arena_from_texts(flat)
    assert offs.size == 2 * len(pairs) + 1
    np.testing.assert_array_equal(offs, o2)
    np.testing.assert_array_equal(arena, a2)


def test_arrow_two_columns_interleave(monkeypatch):
    import pyarrow as pa  # (plainly: a missing library fails, it does not skip)
    from streaming_data_loader_amd import arrow_io
    prem = ["a b", "", "héllo wörld", "x" * 300, "tail"]
    hyp = ["c", "中文", "", "y" * 17, ""]
    labels = [1, 0, 2, 1, 0]
    rb = pa.record_batch([pa.array(prem, pa.utf8()), pa.array(hyp, pa.utf8()), pa.array(labels, pa.int64())],
                         names=["premise", "hypothesis", "label"])
    for batch in (rb, rb.slice(1, 3)):
        k = batch.num_rows
        p, h = batch.column(0).to_pylist(), batch.column(1).to_pylist()
        a = arrow_io.arena_from_batch(batch, "premise", "label", alt_column="hypothesis")
        assert a.n_records == 2 * k and a.label_offsets.size == k + 1
        flat = [t for pr in zip(p, h) for t in pr]
        body = a.arena[:int(a.offsets[-1])].tobytes()
        assert body == "".join(flat).encode("utf-8")
        lens = np.diff(a.offsets.astype(np.int64))
        assert lens.tolist() == [len(t.encode("utf-8")) for t in flat]
        assert a.arena.size >= body.__len__() + 16
    # nulls read as empty text, on either side
    rb2 = pa.record_batch([pa.array(["a", None, "c"], pa.utf8()), pa.array([None, "b", "d"], pa.utf8()),
                           pa.array([0, 1, 0], pa.int64())], names=["premise", "hypothesis", "label"])
    a = arrow_io.arena_from_batch(rb2, "premise", "label", alt_column="hypothesis")
    assert a.arena[:int(a.offsets[-1])].tobytes() == b"abcd"
    assert a.offsets.tolist() == [0, 1, 1, 1, 2, 3, 4]
    # the single-column reader over null rows whose slots hold bytes (a filtered array keeps them)
    col = pa.Array.from_buffers(pa.utf8(), 4, [pa.py_buffer(bytes([0b1101])), pa.py_buffer(np.array([0, 2, 5, 6, 9], np.int32)),
                                               pa.py_buffer(b"aaXXXbccc")])
    assert col.to_pylist() == ["aa", None, "b", "ccc"]
    rb3 = pa.record_batch([col, pa.array([0, 1, 2, 3], pa.int64())], names=["text", "label"])
    a = arrow_io.arena_from_batch(rb3, "text", "label")
    assert a.arena[:int(a.offsets[-1])].tobytes() == b"aabccc" and a.offsets.tolist() == [0, 2, 2, 3, 6]
    # the gather in several steps gives what one step gives (rows longer than a step go alone)
    rng = random.Random(2)
    big_a = ["".join(rng.choice("ab é中") for _ in range(rng.choice([0, 1, 7, 60]))) for _ in range(300)]
    big_b = ["".join(rng.choice("xy z") for _ in range(rng.choice([0, 3, 25, 200]))) for _ in range(300)]
    rb4 = pa.record_batch([pa.array(big_a, pa.utf8()), pa.array(big_b, pa.utf8()), pa.array([0] * 300, pa.int64())],
                          names=["premise", "hypothesis", "label"])
    one = arrow_io.arena_from_batch(rb4, "premise", "label", alt_column="hypothesis")
    monkeypatch.setattr(arrow_io, "_GATHER_BLOCK", 50)
    for batch in (rb4, rb4.slice(17, 200)):
        many = arrow_io.arena_from_batch(batch, "premise", "label", alt_column="hypothesis")
        flat = [t for pr in zip(batch.column(0).to_pylist(), batch.column(1).to_pylist()) for t in pr]
        assert many.arena[:int(many.offsets[-1])].tobytes() == "".join(flat).encode("utf-8")
        assert np.diff(many.offsets.astype(np.int64)).tolist() == [len(t.encode("utf-8")) for t in flat]
    np.testing.assert_array_equal(one.arena, arrow_io.arena_from_batch(rb4, "premise", "label",
                                                                       alt_column="hypothesis").arena)


def test_simple_batcher_pair_argument_checks():
    """The mirror's own checks need no handle: alt_text and the label kind."""
    from streaming_data_loader_amd import batcher as B
    assert B.SingleClass().pair is False and B.MultiLabel(9).pair is False
    assert B.SingleClass(pair=True).pair and B.MultiLabel(5, pair=True).pair
    c, kind = B._native_config(B.BatchConfig(4, 16), B.SingleClass(pair=True), False, 0, 0, 0, 0)
    assert c.pair == 1 and kind == "bert-single"
    c, _ = B._native_config(B.BatchConfig(4, 16), B.MultiLabel(3), False, 0, 0, 0, 0)
    assert c.pair == 0
