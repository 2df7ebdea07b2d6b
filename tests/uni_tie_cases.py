"""The inputs of the tied-score Unigram tests, built the same way with and without a device
(test infrastructure: tests/test_t5_tied_scores.py runs every builder on the CPU -- census
conditions, plain model == oracle, how many words each wrong variant of the model changes --
and tests/test_gpu_unigram_ties.py sends the same records through the HIP kernels).

A builder takes a vocabulary context -- `census` (uni_census.Census), `tok` (the C oracle),
`model` (unigram_plain_model.PlainUnigram), `parts` / `lower` (printable-ASCII plain pieces),
`cat` and `chunks` as test_gpu_unigram_paths.Dev has them -- and returns a Case:

  path     the path class the case is about, the one its census assertion names
  blobs    the records (whole 1 KiB chunks where the case is about a chunk)
  guard    the words of the case the plain model can take (normalization is the identity)
  census   callable(cs): asserts, on the census of the blobs' chunks, that the words sit on
           that path

Words are strings, so one seeded set of word lists (Words) serves every vocabulary: 150
lower-case word-table misses of 4..16 bytes, 150 simple words of 17..48, 60 of 49..128, 10 of
129..512, 8 past 512, each a concatenation of proxy pieces.  The `>=` variant of the model
changes 5..90 % of any of them on any tied vocabulary; the f32-only and reversed-sum variants
change 1..2 % on `u2`, so Words also searches (seeded, at most SEARCH words a class) a few
words on which those two differ and appends them to the lists.
"""
import json
import os
import random

import make_t5_long_piece_vocab as lp
import make_t5_tied_vocab as tv
import oracle_lib
import uni_census
from test_gpu_unigram_paths import ARENA_MAX, CH, K, Dev, embed, rec, fit_lens
from unigram_plain_model import PlainUnigram

VOCABS = (("proxy", "flat"), ("proxy", "g2"), ("proxy", "u2"), ("proxy", "u05"),
          ("v19", "u2"), ("v32", "g2"), ("v64", "flat"))
SEARCH = 2000
WM, VM = K["UNI_WMAX"], K["UNI_VMAX"]
# characters whose normalization is the identity: with a one-char piece, and with no piece at all
WITH_PIECE = "éñöüáà"
NO_PIECE = "中ßøк€한"


def write_vocab(dirpath, base, kind):
    path = os.path.join(str(dirpath), "tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(tv.build(kind, base), f, ensure_ascii=False)
    return path


def equip(ctx, path, base, kind):
    """What the builders need beside Dev's census / tok / parts / cat / chunks."""
    ctx.path, ctx.base, ctx.kind, ctx.name = path, base, kind, f"{base}-{kind}"
    ctx.model = PlainUnigram.from_file(path)
    ctx.lower = [p for p in ctx.parts if p.isalpha() and p.islower()]
    ctx.plan = lp.plan(base) if base != "proxy" else {"plain": [], "meta": []}
    ctx.new = set(lp.new_ids(base).values()) if base != "proxy" else set()
    return ctx


class Host:
    """A vocabulary without a device: Dev minus its DeviceBatcher."""

    def __init__(self, path, base, kind):
        with open(path, encoding="utf-8") as f:
            vocab = json.load(f)["model"]["vocab"]
        self.census = uni_census.Census(vocab)
        self.tok = oracle_lib.T5Tok(path)
        self.parts = [p for p, _ in vocab[3:32000] if not p.startswith("▁") and len(p) <= 16 and
                      all(0x21 <= ord(c) <= 0x7E and c not in "<>" for c in p)]
        equip(self, path, base, kind)

    cat, chunks = Dev.cat, Dev.chunks


class Case:
    def __init__(self, path, blobs, guard, census):
        self.path, self.blobs, self.guard, self.census = path, blobs, guard, census


def differs(model, w, **switch):
    return model.encode_word(w, **switch) != model.encode_word(w)


def search(gen, pred, want, limit=SEARCH):
    """The first `want` words of at most `limit` draws of gen() that pred accepts; (words, draws)."""
    out, n = [], 0
    while len(out) < want and n < limit:
        w = gen()
        n += 1
        if w not in out and pred(w):
            out.append(w)
    return out, n


def lower_miss(ctx, rng, n):
    """A lower-case concatenation of lower-case pieces of n bytes that no word-table rule produces."""
    while True:
        s = ""
        while len(s) < n:
            s += rng.choice(ctx.lower)
        if ctx.census.clear_miss(s[:n]):
            return s[:n]


class Words:
    """The seeded word lists, and what the searches on the `u2` model found (`found`: class ->
    {switch: (words found, words drawn)})."""

    CLASSES = (("narrow", 4, WM, 150, 3, 2), ("wide", WM + 1, VM, 150, 3, 2),
               ("long1", VM + 1, K["LONG_NORM1"], 60, 1, 0),
               ("long2", K["LONG_NORM1"] + 1, K["LONG_NORM"], 10, 1, 0),
               ("huge", K["LONG_NORM"] + 1, 700, 8, 1, 0))

    def __init__(self, u2):
        assert (u2.base, u2.kind) == ("proxy", "u2")
        rng = random.Random(1602)
        self.found = {}
        for name, lo, hi, n, n_f32, n_rev in self.CLASSES:
            if name == "narrow":
                def gen():
                    return lower_miss(u2, rng, rng.randint(lo, hi))
            else:
                def gen():
                    return u2.cat(rng, rng.randint(lo, hi))
            words = []
            while len(words) < n:
                w = gen()
                if w not in words:
                    words.append(w)
            self.found[name] = {}
            for switch, want in (("f32", n_f32), ("reverse_sum", n_rev)):
                hot, drawn = search(gen, lambda w: differs(u2.model, w, **{switch: True}), want)
                self.found[name][switch] = (hot, drawn)
                words += [w for w in hot if w not in words]
            setattr(self, name, words)
        # more than UNI_VPC short misses for one chunk
        self.narrow_over = []
        for n in fit_lens(K["UNI_VPC"] + 2, 4, 9):
            w = lower_miss(u2, rng, n)
            while w in self.narrow_over:
                w = lower_miss(u2, rng, n)
            self.narrow_over.append(w)


def pack(words, max_words=10 ** 6, max_units=10 ** 6, room=CH - 1):
    """Records of one chunk each, words in order: at most max_words words, max_units 16-byte
    payload units and `room` bytes a record."""
    out, cur, size, units = [], [], 0, 0
    for w in words:
        n = len(w.encode())
        u = (n + 15) // 16
        assert n <= room
        if cur and (size + 1 + n > room or len(cur) + 1 > max_words or units + u > max_units):
            out.append(cur)
            cur, size, units = [], 0, 0
        size += n + (1 if cur else 0)
        units += u
        cur.append(w)
    if cur:
        out.append(cur)
    blobs = [rec(ws) for ws in out]
    assert all(len(b) == CH for b in blobs)
    return blobs, out


# ---- word-table hits ---------------------------------------------------------------------------

def table_case(ctx, W=None):
    """Words w, "w," and "w." with "▁w" a piece: the ids are the host's Viterbi at load.  30 seeded
    lower-case w, then, from one pass over all such w in the same seeded order, the first 15 whose
    ids the `>=` variant of the model changes and the first 5 whose ids the f32-only variant
    changes.  ("▁w" is a piece, so few w have a tied split: 31 on g2, 13 on u2, 3 on u05 and
    none on flat, where one piece beats every split; the f32-only variant changes 10 on u2.)"""
    rng = random.Random(316)
    base = sorted(w for w in ctx.census.base if w.isalpha() and w.islower() and 3 <= len(w) < WM)
    rng.shuffle(base)
    forms = lambda w: [w, w + ",", w + "."]  # noqa: E731
    ws = base[:30]
    hot = {"strict": [], "f32": []}
    nudged = ctx.kind in ("u2", "u05")  # f32 scores only differ from the f64 ones where nudged
    for w in base[30:]:
        good = ctx.model.encode_word(w)
        if len(hot["strict"]) < 15 and ctx.model.encode_word(w, strict=False) != good:
            hot["strict"].append(w)
        if nudged and len(hot["f32"]) < 5 and ctx.model.encode_word(w, f32=True) != good:
            hot["f32"].append(w)
    ws += hot["strict"] + [w for w in hot["f32"] if w not in hot["strict"]]
    words = [f for w in ws for f in forms(w)]
    blobs, _ = pack(words, max_words=80)

    def census(cs):
        assert sum(c["hits"] for c in cs) >= len(words)  # (the filler words are hits too)
        assert all(c["narrow"] == c["wide"] == c["medium"] == c["long"] == 0 for c in cs)
        assert all(ctx.census.in_word_table(w) for w in words)
    return Case("word table", blobs, words, census)


# ---- narrow jobs ----------------------------------------------------------------------------------

def narrow_case(ctx, W):
    """Word-table misses of 4..UNI_WMAX bytes: chunks within UNI_VPC jobs, and one over it (the
    losers become long items)."""
    blobs, per = pack(W.narrow, max_words=60)
    over = rec(W.narrow_over)
    assert len(over) == CH

    def census(cs):
        assert [c["narrow"] for c in cs] == [len(p) for p in per] + [K["UNI_VPC"] + 2]
        assert all(c["narrow"] <= K["UNI_VPC"] for c in cs[:-1]) and cs[-1]["narrow"] > K["UNI_VPC"]
        assert all(c["wide"] == c["medium"] == c["long"] == 0 and c["units"] == c["narrow"] for c in cs)
        assert all(ctx.census.clear_miss(w) and 4 <= len(w) <= WM for w in W.narrow + W.narrow_over)
    return Case("narrow", blobs + [over], W.narrow + W.narrow_over, census)


# ---- wide jobs (vocabularies that keep the wide Viterbi) -------------------------------------------

def long_piece_words(ctx, rng, lo, hi):
    """The vocabulary's new plain pieces (v19 / v32 / v64) alone or inside words of lo..hi bytes."""
    out = []
    for p in ctx.plan["plain"]:
        if len(p) > hi:
            continue
        total = rng.randint(max(lo, len(p)), hi)
        out.append(embed(ctx, rng, p, rng.randint(0, total - len(p)), total))
    return out


def wide_case(ctx, W):
    """Simple words of UNI_WMAX+1..UNI_VMAX bytes, every chunk with more than PFX_JOBS of them
    (several passes of k_unigram_viterbi<true>) and within the payload units."""
    assert ctx.census.wide_ok
    words = W.wide + long_piece_words(ctx, random.Random(1948), WM + 1, VM)
    blobs, per = pack(words, max_units=K["UNI_VPC"])

    def census(cs):
        assert [c["wide"] for c in cs] == [len(p) for p in per]
        assert all(c["long"] == c["medium"] == c["narrow"] == 0 and c["units"] <= K["UNI_VPC"] for c in cs)
        assert all(c["wide"] > K["PFX_JOBS"] for c in cs[:-1])
        assert all(WM < l <= VM for c in cs for l in c["wide_lens"])
    return Case("wide", blobs, words, census)


# ---- medium words -------------------------------------------------------------------------------------

def accented(ctx, rng, chars, lo, hi, n):
    """n words of lo..hi bytes: lower-case pieces around one of `chars`, normalization the identity."""
    out = []
    while len(out) < n:
        c = rng.choice(chars)
        total = rng.randint(lo, hi) - len(c.encode())
        k = rng.randint(0, total)
        src = ctx.lower if hi <= WM else ctx.parts
        cat = lambda m: "".join(rng.choice(src) for _ in range(m))[:m]  # noqa: E731
        w = cat(k) + c + cat(total - k)
        if w not in out and ctx.tok.normalize(w) == w:
            out.append(w)
    return out


def medium_case(ctx, W=None):
    """Words of at most UNI_WMAX bytes with one non-ASCII character that has a piece: normalized
    in the chunk's LDS arena, then the narrow DP.  Within the arena's slots and the queue."""
    words = accented(ctx, random.Random(233), WITH_PIECE, 4, WM, 120)
    blobs, per = pack(words, max_words=K["ARENA"] // WM - 8)

    def census(cs):
        assert [c["medium"] for c in cs] == [len(p) for p in per]
        assert all(c["medium"] <= min(K["ARENA"] // WM, K["MED_CAP"]) for c in cs)
        assert all(c["narrow"] == c["wide"] == c["long"] == 0 for c in cs)
    return Case("medium", blobs, words, census)


# ---- long items and huge words ----------------------------------------------------------------------

def long_case(ctx, W):
    """Words of UNI_VMAX+1..LONG_NORM1 and LONG_NORM1+1..LONG_NORM normalized bytes: the two stages
    of k_unigram_long.  One long item a word, nothing else in the chunks but filler hits."""
    words = W.long1 + W.long2 + long_piece_words(ctx, random.Random(64), VM + 1, 100)
    blobs, _ = pack(words, max_words=6)

    def census(cs):
        assert sum(c["long"] for c in cs) == len(words)
        assert all(c["narrow"] == c["wide"] == c["medium"] == 0 for c in cs)
        assert all(VM < len(w) <= K["LONG_NORM1"] for w in W.long1)
        assert all(K["LONG_NORM1"] < len(w) <= K["LONG_NORM"] for w in W.long2)
    return Case("long", blobs, words, census)


def window_case(ctx, W):
    """Wide-length words that start in a chunk's last bytes: the one whose end the window still
    shows (a wide job where the vocabulary has them), and one byte further (word_len reports 0:
    a long item)."""
    lim = CH + K["HALO_R"] - 8
    words = [w for w in W.wide if len(w) >= 25][:24]
    blobs, kinds = [], []
    for i, w in enumerate(words):
        end = lim - (i % 2 == 0)  # lim - 1: in sight; lim: out of sight
        start = end - len(w)
        assert CH - VM <= start < CH
        blobs.append(rec(rec(["the"] * 50)[:start - 1] + b" " + w.encode() + b" "))
        kinds.append("wide" if i % 2 == 0 and ctx.census.wide_ok else "long")

    def census(cs):
        assert all(len(b) == 2 * CH for b in blobs) and kinds.count("long") >= 4
        assert [("wide" if c["wide"] else "long") for c in cs[::2]] == kinds
        assert all(c["wide"] + c["long"] == 1 for c in cs[::2]) and all(c["wide"] + c["long"] == 0 for c in cs[1::2])
    return Case("long (end out of the window's sight)", blobs, words, census)


def long_variant_case(ctx, W):
    """v32 / v64: the wide Viterbi is off, every 17..48-byte word is a long item of
    k_unigram_long<32> / <64>."""
    assert not ctx.census.wide_ok
    words = W.wide + long_piece_words(ctx, random.Random(3264), WM + 1, VM)
    blobs, _ = pack(words, max_words=16)

    def census(cs):
        assert all(c["wide"] == c["narrow"] == c["medium"] == 0 for c in cs)
        assert sum(c["long"] for c in cs) == len(words) and all(WM < len(w) <= VM for w in words)
    return Case("long (17..48 bytes, wide Viterbi off)", blobs, words, census)


def huge_case(ctx, W):
    """Words past LONG_NORM normalized bytes: k_unigram_huge."""
    blobs = [rec([w]) for w in W.huge]

    def census(cs):
        assert sum(c["long"] for c in cs) == len(W.huge) and all(len(w) > K["LONG_NORM"] for w in W.huge)
        assert all(c["narrow"] == c["wide"] == c["medium"] == 0 for c in cs)
    return Case("huge", blobs, W.huge, census)


# ---- unks --------------------------------------------------------------------------------------------

def unk_case(ctx, W=None):
    """Words that mix pieces with characters that have no piece (each an unk of min - 10, on the
    grid of g2 / u2), through the medium path (<= UNI_WMAX bytes) and as long items (17..48
    bytes but not simple, and 49..128 bytes).  The unk's score enters every sum past it; it never
    competes with a piece at its own start (every character that starts a proxy piece is a
    one-char piece), so "the unk is tried last" decides nothing here."""
    rng = random.Random(2600)
    med = accented(ctx, rng, NO_PIECE, 5, WM, 80)
    two = [a[:7] + rng.choice(NO_PIECE) + b[:5] for a, b in zip(med[::2], med[1::2])]
    two = [w for w in two if len(w.encode()) <= WM and ctx.tok.normalize(w) == w]
    long_ = accented(ctx, rng, NO_PIECE, WM + 1, VM, 40) + accented(ctx, rng, NO_PIECE, VM + 1, 128, 40)
    long_ += [a + rng.choice(NO_PIECE) + b for a, b in zip(long_[::4], long_[1::4])]
    long_ = [w for w in long_ if ctx.tok.normalize(w) == w]
    mb, mper = pack(med + two, max_words=K["ARENA"] // WM - 8)
    lb, _ = pack(long_, max_words=8)
    words = med + two + long_

    def census(cs):
        assert [c["medium"] for c in cs[:len(mb)]] == [len(p) for p in mper]
        assert all(c["long"] == 0 for c in cs[:len(mb)]) and all(c["medium"] == 0 for c in cs[len(mb):])
        assert sum(c["long"] for c in cs[len(mb):]) == len(long_)
        assert all(c["narrow"] == c["wide"] == 0 for c in cs)
        for w in words:  # the character is an unk of its own: no piece holds it
            assert ctx.model.unk_id in ctx.model.encode_word(w)
    return Case("medium and long, through unks", mb + lb, words, census)


# ---- records for the task / entry point cases ---------------------------------------------------------

def mixed_records(W, seed, n=24):
    """Short records of words of every class (no huge one): narrow, wide and long words between
    in-vocabulary words, 150..900 bytes each."""
    rng = random.Random(seed)
    pool = W.narrow + W.wide + W.long1[:20] + ["the", "of", "and", "data,", "model."] * 20
    out = []
    for _ in range(n):
        k = rng.randint(8, 40)
        out.append(" ".join(rng.choice(pool) for _ in range(k)).encode())
    return out


def guard_counts(ctx, words, switches=("strict", "f32", "reverse_sum")):
    """{switch: number of `words` on which that wrong variant of the model changes the ids},
    after asserting that the model itself equals the oracle on every word."""
    good = {}
    for w in words:
        good[w] = ctx.model.encode_word(w)
        assert good[w] == ctx.tok.encode(w)[:-1], (ctx.name, w)
    out = {}
    for s in switches:
        kw = {"strict": False} if s == "strict" else {s: True}
        out[s] = sum(ctx.model.encode_word(w, **kw) != good[w] for w in good)
    return out


# ---- which case runs on which vocabulary ---------------------------------------------------------------
PROXIES = ("proxy-flat", "proxy-g2", "proxy-u2", "proxy-u05")
CASES = {
    "table": (table_case, PROXIES),
    "narrow": (narrow_case, PROXIES),
    "wide": (wide_case, PROXIES + ("v19-u2",)),
    "medium": (medium_case, PROXIES),
    "long": (long_case, PROXIES + ("v19-u2", "v32-g2", "v64-flat")),
    "window": (window_case, PROXIES[:3] + ("v19-u2", "v32-g2")),
    "long_variant": (long_variant_case, ("v32-g2", "v64-flat")),
    "huge": (huge_case, PROXIES + ("v64-flat",)),
    "unk": (unk_case, ("proxy-g2", "proxy-u2")),
}
CASE_PARAMS = [(c, v) for c, (_, vs) in CASES.items() for v in vs]
