#!/usr/bin/env python3
"""Build the offline *proxy* bert-base-cased tokenizer asset.

The cased sibling of tools/make_proxy_assets.py: the same trainer over the same corpus
(the fixture records and English docstrings of the locally installed Python packages) plus
the held-out records (tests/golden/heldout_records.jsonl), so that accented letters of both
cases get pieces; normalized by BertNormalizer(lowercase=False, strip_accents=False).  The
vocabulary has bert-base-cased's size (28,996) and its special-id layout:

    [PAD]=0  [unused1..99]=1..99  [UNK]=100  [CLS]=101  [SEP]=102  [MASK]=103
    [unused100..101]=104..105    learned pieces 106..28995

Output (committed): tests/golden/bert_normalizer/bert_cased_proxy_vocab.txt.gz, the vocab.txt.
build() installs it, with the tokenizer.json around it (build.py cased_tokenizer_json: what
BertWordPieceTokenizer saves for it), as
  streaming_data_loader_amd/assets/bert_cased_proxy/vocab.txt
  streaming_data_loader_amd/assets/bert_cased_proxy/tokenizer.json

The other two normalizer settings the WordPiece path takes (lowercase with kept accents,
cased with stripped accents) reuse this vocabulary: the tests flip the two normalizer
fields of the installed tokenizer.json.

The script asserts that the vocabulary holds what the cased kernel's tests need -- pieces
with ASCII capitals on both sides of the first-piece table's 14-byte limit, "##" pieces
with capitals, pieces with non-ASCII letters of both cases -- and prints the counts.
"""
import gzip
import json
import os
import sys

from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, trainers
from tokenizers.implementations import BertWordPieceTokenizer

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_proxy_assets import docstring_corpus, fixture_texts  # noqa: E402

REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
from streaming_data_loader_amd import build  # noqa: E402

OUT = os.path.join(REPO, "streaming_data_loader_amd", "assets", "bert_cased_proxy")
HELDOUT = os.path.join(REPO, "tests", "golden", "heldout_records.jsonl")

VOCAB_SIZE = 28996
N_RESERVED = 106  # [PAD] + [unused1..99] + 4 specials + [unused100..101]  (ids 0..105)


def heldout_texts():
    with open(HELDOUT, "r", encoding="utf-8") as f:
        return [json.loads(l)["text"] for l in f]


def counts(vocab):
    def has_cap(s):
        return any("A" <= c <= "Z" for c in s)

    first = [p for p in vocab[N_RESERVED:] if not p.startswith("##")]
    cont = [p[2:] for p in vocab[N_RESERVED:] if p.startswith("##")]
    na = [p for p in first + cont if any(ord(c) >= 0x80 and c.isalpha() for c in p)]
    return {
        "first_caps_le14": sum(1 for p in first if p.isascii() and has_cap(p) and len(p) <= 14),
        "first_caps_ge15": sum(1 for p in first if p.isascii() and has_cap(p) and len(p) >= 15),
        "cont_caps": sum(1 for p in cont if has_cap(p)),
        "nonascii_upper": sum(1 for p in na if any(ord(c) >= 0x80 and c.isupper() for c in p)),
        "nonascii_lower": sum(1 for p in na if any(ord(c) >= 0x80 and c.islower() for c in p)),
    }


def main():
    os.makedirs(OUT, exist_ok=True)
    texts = fixture_texts() * 40 + docstring_corpus() + heldout_texts() * 40
    specials = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    tok = Tokenizer(models.BPE(unk_token="[UNK]", continuing_subword_prefix="##"))
    tok.normalizer = normalizers.BertNormalizer(lowercase=False, strip_accents=False)
    tok.pre_tokenizer = pre_tokenizers.BertPreTokenizer()
    n_learn = VOCAB_SIZE - N_RESERVED
    trainer = trainers.BpeTrainer(vocab_size=n_learn + len(specials) + 64,
                                  special_tokens=specials, min_frequency=2,
                                  limit_alphabet=1000, continuing_subword_prefix="##",
                                  max_token_length=18)
    tok.train_from_iterator(texts, trainer)
    learned = sorted(tok.get_vocab().items(), key=lambda kv: kv[1])
    learned = [t for t, _ in learned if t not in specials][:n_learn]
    assert len(learned) == n_learn, len(learned)
    vocab = ["[PAD]"] + [f"[unused{i}]" for i in range(1, 100)] + ["[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    vocab += ["[unused100]", "[unused101]"]
    assert len(vocab) == N_RESERVED
    vocab += learned
    assert len(vocab) == VOCAB_SIZE and len(set(vocab)) == VOCAB_SIZE
    os.makedirs(os.path.dirname(build.CASED_VOCAB_GZ), exist_ok=True)
    with open(build.CASED_VOCAB_GZ, "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:
            g.write(("\n".join(vocab) + "\n").encode("utf-8"))
    build.install_assets()
    saved = os.path.join(OUT, "saved.json")
    BertWordPieceTokenizer(os.path.join(OUT, "vocab.txt"), lowercase=False, clean_text=True,
                           handle_chinese_chars=True, strip_accents=False).save(saved)
    with open(saved, encoding="utf-8") as f, open(os.path.join(OUT, "tokenizer.json"), encoding="utf-8") as g:
        assert json.load(f) == json.load(g)  # the installed tokenizer.json is what tokenizers saves
    os.remove(saved)
    t = Tokenizer.from_file(os.path.join(OUT, "tokenizer.json"))
    for s, want in (("[PAD]", 0), ("[UNK]", 100), ("[CLS]", 101), ("[SEP]", 102), ("[MASK]", 103)):
        assert t.token_to_id(s) == want, (s, t.token_to_id(s))
    c = counts(vocab)
    assert all(v > 0 for v in c.values()), c
    enc = t.encode(fixture_texts()[0])
    print("vocab", len(vocab), "longest piece", max(len(p.encode()) for p in vocab), "bytes;",
          " ".join(f"{k}={v}" for k, v in c.items()), "first ids", enc.ids[:12], file=sys.stderr)


if __name__ == "__main__":
    main()
