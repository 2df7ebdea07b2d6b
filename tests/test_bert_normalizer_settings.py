"""BertNormalizer settings beside bert-base-uncased's (CPU): cased (lowercase=false,
strip_accents=false), uncased with kept accents (true, false) and cased with stripped accents
(false, true).

- each setting's Unicode table (tests/golden/bert_normalizer/bert_*_unicode.bin, installed into
  streaming_data_loader_amd/data/ by build()) re-probed
  through tokenizers' BertNormalizer: all of ASCII and Latin-1 and a seeded sample;
- the C oracle on the cased proxy vocabulary and that table against tokenizers'
  BertWordPieceTokenizer, over the fixture records, the held-out records and the records the
  GPU test generates (wp_cased_cases.py): no text may differ;
- the host loader (sdl_tokenizer_info_get): the three settings load and report their
  normalizer_flags, what loaded before reports 0, clean_text / handle_chinese_chars false
  stay refused by name.

The cased proxy vocabulary (tools/make_proxy_cased_assets.py, 28,996 pieces, longest 21
bytes) holds, of non-"##" ASCII pieces with a capital, 8,036 of <= 14 bytes and 67 of >= 15
bytes; 1,478 "##" pieces with a capital; 38 pieces with a non-ASCII upper-case letter and 376
with a non-ASCII lower-case one."""
import json
import os
import random
import struct

import numpy as np
import pytest
import tokenizers
from tokenizers.implementations import BertWordPieceTokenizer

import oracle_lib
import wp_cased_cases as W
from streaming_data_loader_amd import native


@pytest.fixture(scope="module")
def cases():
    return W.Cases()


def test_installed_tokenizer_json_is_what_tokenizers_saves(native_lib, tmp_path):
    """build() writes the cased proxy's tokenizer.json itself, around the committed vocabulary:
    it is what BertWordPieceTokenizer(vocab.txt, lowercase=False, strip_accents=False) saves.
    The installed vocab.txt and tables are the committed ones."""
    with open(W.CASED_VOCAB, "rb") as f, open(os.path.join(os.path.dirname(native.BERT_CASED_PROXY_TOKENIZER),
                                                         "vocab.txt"), "rb") as g:
        assert f.read() == g.read()
    for setting in W.SETTINGS:
        src = W.SETTINGS[setting][2]
        with open(src, "rb") as f, open(os.path.join(native.DATA_DIR, os.path.basename(src)), "rb") as g:
            assert f.read() == g.read()
    out = tmp_path / "saved.json"
    BertWordPieceTokenizer(W.CASED_VOCAB, lowercase=False, strip_accents=False).save(str(out))
    with open(native.BERT_CASED_PROXY_TOKENIZER, encoding="utf-8") as f:
        assert json.load(f) == json.loads(out.read_text(encoding="utf-8"))
    v = W.vocab()
    assert len(v) == 28996 and [v[i] for i in (0, 100, 101, 102, 103)] == ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]


def read_table(path):
    d = open(path, "rb").read()
    magic, ver, npg, nbl, pl = struct.unpack("<4sIIII", d[:20])
    assert magic == b"SDLU" and ver == 2 and len(d) == 20 + 2 * npg + 4 * 128 * nbl + pl
    pages = np.frombuffer(d, np.uint16, npg, 20)
    ent = np.frombuffer(d, np.uint32, nbl * 128, 20 + 2 * npg)
    return pages, ent, d[20 + 2 * npg + 4 * 128 * nbl:]


@pytest.mark.parametrize("setting", sorted(W.SETTINGS))
def test_table_probe_sample(setting, cases):
    lower, strip, path, _ = W.SETTINGS[setting]
    norm = tokenizers.normalizers.BertNormalizer(lowercase=lower, strip_accents=strip)
    pages, ent, pool = read_table(path)
    rng = random.Random(11)
    cps = list(range(0x100)) + [rng.randrange(0x100, 0x110000) for _ in range(4000)]
    # (the chars the GPU records lean on, whatever the sample holds)
    cps += [ord(c) for w in cases.w16_words + cases.long_words for c in w if ord(c) >= 0x100]
    cps += [ord(c) for c in W.HI + W.LO + W.M9]
    for cp in cps:
        if 0xD800 <= cp <= 0xDFFF:
            continue
        e = int(ent[int(pages[cp >> 7]) * 128 + (cp & 127)])
        n = norm.normalize_str(chr(cp))
        core = n.replace(" ", "")
        if (e & 3) == 3:
            assert n == "", hex(cp)
        elif (e & 3) == 1:
            assert n.strip() == "" or all(c.isspace() for c in n), hex(cp)
        else:
            mapped = chr(cp) if e & 4 else pool[(e >> 8) + 2:(e >> 8) + 2 + pool[e >> 8]].decode()
            assert mapped == core, (hex(cp), mapped, core)
    # ASCII letters: lower-cased by a lower-casing table, themselves in a cased one
    for c in range(ord("A"), ord("Z") + 1):
        e = int(ent[int(pages[0]) * 128 + c])
        assert bool(e & 4) == (not lower)
    # a setting that keeps accents reorders nothing: no canonical-ordering flag at all
    flagged = int(np.count_nonzero(ent & 16))
    assert (flagged == 0) if not strip else (flagged > 0)


@pytest.mark.parametrize("setting", sorted(W.SETTINGS))
def test_oracle_matches_tokenizers(setting, records, cases):
    lower, strip, _, _ = W.SETTINGS[setting]
    tok = W.oracle(setting)
    hf = BertWordPieceTokenizer(W.CASED_VOCAB, lowercase=lower, strip_accents=strip)
    texts = records + W.heldout_texts() + cases.texts
    differ = [i for i, t in enumerate(texts) if tok.encode(t) != hf.encode(t).ids]
    assert not differ, f"{len(differ)} of {len(texts)} texts differ, first {differ[:5]}"
    cases.check_setting(setting, tok)


def test_oracle_matches_tokenizers_on_reordered_marks(native_lib, tmp_path, cases):
    """Canonical ordering shows in the ids only with pieces for the kept marks: with them in
    three [unused] slots, cased + stripped accents sorts a run of marks by ccc (both orders
    give the same ids), the settings without NFD leave the run as it came."""
    words = [w for p in cases.reorder_pairs for w in p]
    for setting in sorted(W.SETTINGS):
        lower, strip, _, _ = W.SETTINGS[setting]
        _, vpath = W.write_tokenizer(tmp_path, setting, mark_pieces=True)
        tok = W.oracle(setting, vpath)
        hf = BertWordPieceTokenizer(vpath, lowercase=lower, strip_accents=strip)
        for w in words:
            assert tok.encode(w) == hf.encode(w).ids, (setting, w)
        for a, b in cases.reorder_pairs:
            assert W.UNK not in W.word_ids(tok, b)
            assert (tok.encode(a) == tok.encode(b)) == strip, (setting, a)


def test_generated_records_are_not_vacuous(cases):
    """Under each cased setting every record's expected row holds a piece with a capital; under
    every setting the expected rows are not the uncased table's."""
    plain = W.framed_rows(oracle_lib.Tok(W.CASED_VOCAB, oracle_lib.UNICODE_BIN), cases.texts, 512)
    for setting in sorted(W.SETTINGS):
        tok = W.oracle(setting)
        if setting in W.CASED_SETTINGS:
            for k, t in enumerate(cases.texts):
                assert any(W.has_capital(cases.V[i]) for i in W.word_ids(tok, t)), (setting, k)
        want = W.framed_rows(tok, cases.texts, 512)
        assert want.shape != plain.shape or (want != plain).any(), setting


@pytest.mark.parametrize("setting", sorted(W.SETTINGS))
def test_loader_accepts_setting(native_lib, tmp_path, setting):
    path, _ = W.write_tokenizer(tmp_path, setting)
    info = native.tokenizer_info(path)
    assert info.kind == 0 and info.vocab_size == 28996 and info.unk_id == W.UNK
    assert info.normalizer_flags == W.SETTINGS[setting][3]


def test_loader_null_strip_accents_follows_lowercase(native_lib, tmp_path):
    for setting, flags in (("cased", 3), ("uncased_accents", 0)):
        path, _ = W.write_tokenizer(tmp_path, setting, strip_accents=None)
        assert native.tokenizer_info(path).normalizer_flags == flags


def test_loader_flags_of_what_loaded_before(native_lib):
    assert native.tokenizer_info(native.BERT_CASED_PROXY_TOKENIZER).normalizer_flags == 3
    for path in (native.BERT_PROXY_TOKENIZER, native.GPT2_PROXY_TOKENIZER, native.T5_PROXY_TOKENIZER,
                 oracle_lib.VOCAB_TXT):
        info = native.tokenizer_info(path)
        assert info.normalizer_flags == 0 and not any(info.reserved)


@pytest.mark.parametrize("option", ["clean_text", "handle_chinese_chars"])
def test_loader_refuses_by_name(native_lib, tmp_path, option):
    path, _ = W.write_tokenizer(tmp_path, "cased", **{option: False})
    with pytest.raises(native.SDLError, match=option):
        native.tokenizer_info(path)
    with open(native.BERT_PROXY_TOKENIZER, encoding="utf-8") as f:
        tj = json.load(f)
    tj["normalizer"][option] = False
    p = tmp_path / "uncased.json"
    p.write_text(json.dumps(tj))
    with pytest.raises(native.SDLError, match=option):
        native.tokenizer_info(str(p))
