"""GPU parity of the WordPiece chunk kernel under the BertNormalizer settings beside
bert-base-uncased's: cased and cased with stripped accents (the kernel's CASED instantiation:
ASCII letters pass word_setup, normalize_w16 and word_materialize unchanged) and uncased with
kept accents (the uncased instantiation on its own table).

Each case runs the 12 generated records of wp_cased_cases.py (about 1,000 bytes each) through
DeviceBatcher with that setting's tokenizer.json -- the cased proxy build() installs, with its two
normalizer fields flipped, written to a temporary directory -- and compares every row with the
C oracle on the cased vocabulary and that setting's table.  The record groups: the fast path
(word / Word / WORD), words around the first-piece table's 14-byte limit, 1, 9 and 40 pending
words a chunk (groups of 8, 4 and 1 lanes), capitals next to non-ASCII letters (normalize_w16),
words of 17..40 bytes and at the 16 | 17 and 96 | 97 byte and 100 | 101 char thresholds (deferred
lattice, general path, [UNK]), kept marks in non-canonical order, a word across arena byte 1024
and one ending with its record, [MASK] and [mask].  What each group claims of its words is
asserted on the CPU (Cases.check_setting, test_bert_normalizer_settings.py).

The cased proxy vocabulary holds 8,036 non-"##" ASCII pieces with a capital of <= 14 bytes, 67
of >= 15 bytes, 1,478 "##" pieces with a capital, 38 pieces with a non-ASCII upper-case letter
and 376 with a non-ASCII lower-case one (tools/make_proxy_cased_assets.py)."""
import numpy as np
import pytest

import oracle_lib
import wp_cased_cases as W
from streaming_data_loader_amd import batcher as Bt
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_parity import framed_rows, run_device, torch  # noqa: F401
from test_gpu_push_direct import drain, planes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return W.Cases()


@pytest.fixture(scope="module")
def plain_rows(cases):
    """The same texts under the uncased table (and the cased vocabulary)."""
    return framed_rows(oracle_lib.Tok(W.CASED_VOCAB, oracle_lib.UNICODE_BIN), cases.texts, 512)


@pytest.mark.parametrize("setting", sorted(W.SETTINGS))
def test_rows_match_oracle(torch, native_lib, tmp_path, cases, plain_rows, setting):  # noqa: F811
    path, _ = W.write_tokenizer(tmp_path, setting)
    tok = W.oracle(setting)
    cases.check_setting(setting, tok)
    want = framed_rows(tok, cases.texts, 512)
    # not vacuous: capitals reach the ids, and the rows are not the uncased table's
    if setting in W.CASED_SETTINGS:
        for k, t in enumerate(cases.texts):
            assert any(W.has_capital(cases.V[i]) for i in W.word_ids(tok, t)), k
    assert want.shape != plain_rows.shape or (want != plain_rows).any()
    db = DeviceBatcher(batch_size=16, sequence_length=512, mask_length=0, min_ids=0, tokenizer=path)
    ids = run_device(torch, db, cases.texts).planes()[0]
    assert ids.shape == want.shape
    bad = np.nonzero((ids != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:5]}"
    db.close()


def test_reordered_marks_match_oracle(torch, native_lib, tmp_path, cases):  # noqa: F811
    """Cased with stripped accents, pieces for the kept marks in three [unused] slots: the
    canonical order of a run of marks shows in the ids (both orders give the same ones)."""
    path, vpath = W.write_tokenizer(tmp_path, "cased_stripped", mark_pieces=True)
    tok = W.oracle("cased_stripped", vpath)
    for a, b in cases.reorder_pairs:
        assert W.UNK not in W.word_ids(tok, b) and W.word_ids(tok, a) == W.word_ids(tok, b)
        assert any(W.has_capital(cases.V[i]) for i in W.word_ids(tok, a))
    texts = [cases.texts[9], " ".join(w for p in cases.reorder_pairs for w in p)]
    want = framed_rows(tok, texts, 512)
    db = DeviceBatcher(batch_size=16, sequence_length=512, mask_length=0, min_ids=0, tokenizer=path)
    ids = run_device(torch, db, texts).planes()[0]
    assert ids.shape == want.shape
    np.testing.assert_array_equal(ids, want)
    db.close()


def test_cased_mlm_planes_match_oracle(torch, native_lib, cases):  # noqa: F811
    tok = W.oracle("cased")
    db = DeviceBatcher(batch_size=16, sequence_length=512, mask_length=76, seed=7,
                       tokenizer=W.native.BERT_CASED_PROXY_TOKENIZER)
    res = run_device(torch, db, cases.texts)
    G = res.rows()
    got = res.planes(G)
    want = oracle_lib.oracle_rows(tok, cases.texts, 512, 76, W.MASK, seed=7, B=16)
    assert want.shape[1] == G and G >= len(cases.texts)
    for j in range(4):
        np.testing.assert_array_equal(got[j], want[j])
    assert (want[3] != -100).any()
    db.close()


def test_cased_per_record_rows_match_oracle(native_lib, cases):
    """The same records one at a time through GenTokenizer (the small-call kernels)."""
    gt = Bt.GenTokenizer(Bt.ModelType.Bert, Bt.BatchConfig(16, 512), Bt.Mask(76, W.MASK),
                         Bt.TokenizerConfig(W.native.BERT_CASED_PROXY_TOKENIZER), chunk=True, seed=7)
    got = planes(drain(gt, cases.texts))
    want = oracle_lib.oracle_rows(W.oracle("cased"), cases.texts, 512, 76, W.MASK, seed=7, B=16)
    assert got[0].shape[0] == want.shape[1]
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
