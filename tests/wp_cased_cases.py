"""Shared by test_bert_normalizer_settings.py (CPU) and test_gpu_wordpiece_cased.py (GPU):
the three BertNormalizer settings next to bert-base-uncased's, their tables, the tokenizer.json
of each (the cased proxy, which build() installs from tests/golden/bert_normalizer/, with its two
normalizer fields flipped, written to a temporary directory) and the generated records.

Every record group is built from the committed cased vocabulary, and the side of a limit a
word is meant to lie on is asserted where the word is chosen (check_*), not hoped for."""
import gzip
import json
import os
import random
import tempfile

import numpy as np

import oracle_lib
from streaming_data_loader_amd import build, native

# The oracle's side reads the committed files: the tables as they lie under
# tests/golden/bert_normalizer/, the vocabulary unpacked into a temporary directory.  The
# product's side (the loader, DeviceBatcher) reads what build() installed from them.
DATA = build.SETTINGS_SRC
_TMP = tempfile.TemporaryDirectory(prefix="bert_cased_proxy_")
CASED_VOCAB = os.path.join(_TMP.name, "vocab.txt")
with gzip.open(build.CASED_VOCAB_GZ, "rb") as _f, open(CASED_VOCAB, "wb") as _g:
    _g.write(_f.read())
HELDOUT = os.path.join(oracle_lib.REPO, "tests", "golden", "heldout_records.jsonl")

# name: (lowercase, strip_accents, table, sdl_tokenizer_info.normalizer_flags)
SETTINGS = {
    "cased": (False, False, os.path.join(DATA, "bert_cased_unicode.bin"), 3),
    "uncased_accents": (True, False, os.path.join(DATA, "bert_uncased_accents_unicode.bin"), 2),
    "cased_stripped": (False, True, os.path.join(DATA, "bert_cased_stripped_unicode.bin"), 1),
}
CASED_SETTINGS = ("cased", "cased_stripped")

UNK, CLS, SEP, MASK = 100, 101, 102, 103
CHUNK = 1024
FIRST_TABLE_MAX = 14  # wp_first.hpp WF_MAXLEN
HI, LO, M9 = "\U0001D16D", "\U0001D165", "᭄"  # kept marks, ccc 226, 216, 9 (make_reorder_goldens.py)
# the canonical-ordering check needs pieces for the kept marks, which no trained vocabulary
# holds: these stand in the slots of [unused1..3]
MARK_PIECES = ["##" + HI, "##" + LO, "##" + M9]

FILLER = "the of and to in a is that for it as was with be by on not he".split()


def vocab():
    with open(CASED_VOCAB, encoding="utf-8") as f:
        return [l.rstrip("\n") for l in f]


def heldout_texts():
    with open(HELDOUT, encoding="utf-8") as f:
        return [json.loads(l)["text"] for l in f]


def tokenizer_json(setting, **normalizer_fields):
    """The installed cased tokenizer.json (build(), the native_lib fixture) as a dict, its
    normalizer set to `setting`."""
    with open(native.BERT_CASED_PROXY_TOKENIZER, encoding="utf-8") as f:
        tj = json.load(f)
    lower, strip = SETTINGS[setting][:2]
    tj["normalizer"]["lowercase"] = lower
    tj["normalizer"]["strip_accents"] = strip
    tj["normalizer"].update(normalizer_fields)
    return tj


def write_tokenizer(dirpath, setting, mark_pieces=False, **normalizer_fields):
    """Writes tokenizer.json (and, with mark_pieces, the vocab.txt the oracle reads) of a
    setting into dirpath; returns (tokenizer.json path, vocab.txt path)."""
    tj = tokenizer_json(setting, **normalizer_fields)
    vpath = CASED_VOCAB
    if mark_pieces:
        v = vocab()
        for k, p in enumerate(MARK_PIECES):
            old = v[1 + k]
            assert old == f"[unused{1 + k}]" and tj["model"]["vocab"][old] == 1 + k
            del tj["model"]["vocab"][old]
            v[1 + k] = p
            tj["model"]["vocab"][p] = 1 + k
        vpath = os.path.join(str(dirpath), f"vocab_{setting}_marks.txt")
        with open(vpath, "w", encoding="utf-8") as f:
            f.write("\n".join(v) + "\n")
    name = f"tokenizer_{setting}{'_marks' if mark_pieces else ''}{''.join('_' + k for k in normalizer_fields)}.json"
    path = os.path.join(str(dirpath), name)
    with open(path, "w", encoding="utf-8") as f:
        json.dump(tj, f, ensure_ascii=False)
    return path, vpath


def oracle(setting, vocab_path=CASED_VOCAB):
    return oracle_lib.Tok(vocab_path, SETTINGS[setting][2])


def word_ids(tok, text):
    """The oracle's ids of a text without the template's [CLS] and [SEP] around them."""
    ids = tok.encode(text)
    assert ids[0] == CLS and ids[-1] == SEP
    return ids[1:-1]


def has_capital(s):
    return any(c.isupper() for c in s)


def framed_rows(tok, texts, S):
    """test_gpu_parity.framed_rows (imported there with torch; restated here for the CPU side)."""
    rows = []
    for t in texts:
        ids = [CLS] + tok.encode(t) + [SEP, SEP]
        for o in range(0, len(ids), S):
            r = np.zeros(S, np.int32)
            c = ids[o:o + S]
            r[:len(c)] = c
            rows.append(r)
    return np.array(rows, np.int32).reshape(-1, S)


class Cases:
    """The 12 generated records and what the tests assert about them."""

    def __init__(self):
        rng = random.Random(0xCA5ED)
        V = vocab()
        S = set(V)
        self.V = V
        tok = oracle("cased")
        first = [p for p in V[106:] if not p.startswith("##")]
        assert all(w in S for w in FILLER)

        # 1. fast path: word / Word / WORD, all pieces of <= 14 bytes
        self.triples = [(w, w.capitalize(), w.upper()) for w in first
                        if w.isascii() and w.isalpha() and w.islower() and 4 <= len(w) <= FIRST_TABLE_MAX and
                        w.capitalize() in S and w.upper() in S][:12]
        assert len(self.triples) == 12

        # 2. in-vocabulary capitalised words around the first-piece table's 14-byte limit
        self.limit_words = []
        for n in (13, 14, 15, 16, 17):
            self.limit_words += [w for w in first if w.isascii() and w.isalpha() and has_capital(w) and len(w) == n][:6]
        assert any(len(w) <= FIRST_TABLE_MAX for w in self.limit_words)
        assert any(len(w) > FIRST_TABLE_MAX for w in self.limit_words)

        # 3. out-of-vocabulary mixed-case ASCII words of 3..16 bytes that end in a capital "##"
        #    piece, in no vocabulary under either case (so they are pending under every setting)
        cont = [p[2:] for p in V if p.startswith("##") and p.isascii() and p[2:].isalpha() and has_capital(p)]
        letters = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
        self.oov = []
        seen = set()
        while len(self.oov) < 80:
            suf = rng.choice(cont)
            n = rng.randint(3, 16)
            if len(suf) >= n:
                continue
            w = "".join(rng.choice(letters) for _ in range(n - len(suf))) + suf
            if w in seen or w in S or w.lower() in S or not has_capital(w) or w.isupper():
                continue
            ids = word_ids(tok, w)
            last = V[ids[-1]]
            if len(ids) < 2 or UNK in ids or not (last.startswith("##") and has_capital(last)):
                continue
            seen.add(w)
            self.oov.append(w)
        assert {len(w) for w in self.oov} >= {3, 16}

        # 4. normalize_w16: capitals next to non-ASCII letters of both cases
        self.w16_words = ["İstanbul", "İSTANBUL", "ΟΔΥΣΣΕΥΣ", "ΌΣΟΣ", "Σίσυφος", "ǅungla", "Xǅ", "Straße", "STRASSE",
                          "GROẞ", "ＡＢc", "Ｆull", "ﬁNal", "Eﬃcient", "AB中CD", "Tokyo東京City", "Don't", "STOP,Go",
                          "U.S.A", "Élan", "éLAN", "ÀÉÎÕÜ", "Ñandú", "Čech", "ŁÓDŹ", "Ångström", "naïveTÉ",
                          "Übergröße", "ÆSIR", "Ðað", "ÞórR"]

        # 5. deferred lattice and general path: 17..40 bytes, then the thresholds -- 16 | 17 bytes
        #    (registers | lattice), 96 | 97 bytes (LW_MAX: lattice | general), 100 | 101 chars
        caps = [w for w in first if w.isascii() and w.isalpha() and has_capital(w) and 5 <= len(w) <= 12]
        self.long_words = []
        while len(self.long_words) < 24:
            w = ""
            target = rng.randint(17, 40)
            while len(w.encode()) < target:
                w += rng.choice(caps) if rng.random() < 0.7 else rng.choice(["É", "ü", "Ö", "ß", "ñ", "Σ", "é"])
            if 17 <= len(w.encode()) <= 40:
                self.long_words.append(w)
        assert any(w.isascii() for w in self.long_words) and any(not w.isascii() for w in self.long_words)

        def mixed(n):  # an n-char mixed-case ASCII word of in-vocabulary letters
            return "".join(rng.choice(letters) for _ in range(n))

        self.sized = {n: mixed(n) for n in (16, 17, 96, 97, 100, 101)}
        self.sized_accented = "É" + mixed(98) + "ß"  # 100 chars, 102 bytes
        assert UNK not in word_ids(tok, self.sized[100]) and word_ids(tok, self.sized[101]) == [UNK]
        assert UNK not in word_ids(tok, self.sized_accented)

        # 6. canonical ordering: two kept marks in non-canonical order beside capitals
        self.reorder_pairs = [("A" + HI + LO, "A" + LO + HI), ("Bc" + LO + M9 + "D", "Bc" + M9 + LO + "D"),
                              ("E" + HI + M9 + LO + "f", "E" + M9 + LO + HI + "f"),
                              ("Gé" + HI + LO + "H", "Gé" + LO + HI + "H")]

        def fill(words, size, pad_to=None):
            """words shuffled among filler, about `size` bytes (exactly pad_to, by spaces)."""
            words = list(words)
            n = sum(len(w.encode()) + 1 for w in words)
            while True:
                f = rng.choice(FILLER)
                if n + len(f) + 1 > size:
                    break
                words.append(f)
                n += len(f) + 1
            rng.shuffle(words)
            s = " ".join(words)
            if pad_to is not None:
                assert len(s.encode()) <= pad_to
                s += " " * (pad_to - len(s.encode()))
            return s

        # 7. seams: record 0 holds an in-vocabulary mixed-case word across arena byte 1024 and
        #    ends, with the record, in a mixed-case word; record 1 starts with a letter
        self.seam_word = next(w for w in self.limit_words if len(w) == 13)
        head = fill(["The", "With"], 1010, pad_to=1017) + " "
        r0 = head + self.seam_word + " " + fill(self.oov[40:44], 60) + " " + self.oov[44]
        self.seam_at = len(head.encode())
        assert self.seam_at < CHUNK < self.seam_at + len(self.seam_word)
        # 1 + 8. the fast path's triples and the added tokens
        r1 = fill([" ".join(t) for t in self.triples] + ["[MASK]", "[mask]", "x[MASK]y", "[MASK].", "[Mask]"], 900,
                  pad_to=2 * CHUNK - len(r0.encode()))
        assert r1[0].isalpha() and r0[-1].isalpha()
        # 3. one chunk each (records 2..4 start at multiples of 1024 and are 1024 bytes long)
        self.pending_counts = (1, 9, 40)
        pend = [fill(self.oov[a:b], 1000, pad_to=CHUNK) for a, b in ((0, 1), (1, 10), (10, 50))]
        r5 = fill(self.limit_words + ["The"], 1000)
        r6 = fill(self.w16_words + ["The", "With"], 1000)
        r7 = fill(self.long_words + ["This"], 1000)
        r8 = fill(list(self.sized.values()) + [self.sized_accented, "That"], 1000)
        r9 = fill([w for p in self.reorder_pairs for w in p] + ["Other", "Class"], 1000)
        pool = (self.limit_words + self.w16_words + self.long_words + self.oov[50:] + [w for t in self.triples for w in t] +
                ["[MASK]", "[mask]", "A" + HI + LO])
        r10 = fill(rng.sample(pool, 60), 1000)
        r11 = fill(rng.sample(pool, 60), 990) + " " + self.oov[45]  # ends without a newline, in a word
        self.texts = [r0, r1] + pend + [r5, r6, r7, r8, r9, r10, r11]
        assert len(self.texts) == 12 and all(900 <= len(t.encode()) <= 1300 for t in self.texts)
        offs = np.cumsum([0] + [len(t.encode()) for t in self.texts])
        arena = "".join(self.texts).encode()
        assert arena[self.seam_at:self.seam_at + len(self.seam_word)] == self.seam_word.encode()
        for k, n in zip((2, 3, 4), self.pending_counts):
            assert offs[k] % CHUNK == 0 and offs[k + 1] - offs[k] == CHUNK
            assert sum(1 for w in self.texts[k].split() if w not in S and w.lower() not in S) == n
            assert all(w in S for w in self.texts[k].split() if w.islower())

    def check_setting(self, setting, tok):
        """What the groups claim, under one setting's oracle: asserted on the CPU."""
        V = self.V
        cased = setting in CASED_SETTINGS
        for t in self.triples:
            ids = [word_ids(tok, w) for w in t]
            assert all(len(i) == 1 for i in ids)
            assert len({i[0] for i in ids}) == (3 if cased else 1), t
        for w in self.limit_words:
            if cased:
                assert word_ids(tok, w) == [V.index(w)]
        assert word_ids(tok, "[MASK]") == [MASK]
        m = word_ids(tok, "[mask]")
        assert len(m) > 1 and MASK not in m
        if cased:
            for w in self.oov:
                last = V[word_ids(tok, w)[-1]]
                assert last.startswith("##") and has_capital(last), w
