"""GPU parity for the Unigram tokenizer's capacity fallbacks and for pieces longer than 16 bytes.

streaming_data_loader_amd/csrc/tokenize_unigram.hip settles a word on one of several paths --
word table, the chunk's own Viterbi jobs (UNI_VPC jobs and 16-byte payload units a chunk), the
medium-word arena (MED_CAP words, ARENA / UNI_WMAX slots), the wide Viterbi (printable ASCII
words of 17..48 bytes, PFX_JOBS a pass, pruned by the `upfx` prefix bound), two long-item
stages (LONG_NORM1 / LONG_NORM normalized bytes) in three instantiations (k_unigram_long
<20|32|64>, chosen from the vocabulary), k_unigram_huge -- and every overflow falls back to a
slower path that must give the same ids.  The other GPU tests reach these by accident; the
cases here are built to sit on a stated side of a stated limit.

Every case
  * asserts its census condition first (tests/uni_census.py: the chunk kernel's classification
    of the input, restated on the host; its limits are read from the kernel sources), so the
    test body says which side of which limit the input is on;
  * compares every record's ids with the CPU oracle (oracle/orc_unigram.c), which
    tests/test_t5_long_pieces.py pins to `tokenizers` on the same vocabularies;
  * asserts the device reported no tokenize error.
Records are 1,024 bytes (or a multiple) where a case is about a chunk, so chunk c is record c.
Ids per record come from CLM rows over the t5 tokenizer (min_ids=0, S=2048), as
test_gpu_span.device_ids reads them; one DeviceBatcher per vocabulary, arenas of <= 64 KiB.

The vocabularies: the t5 proxy asset (no piece past 16 bytes) and the v19 / v32 / v64 variants of
tests/golden/make_t5_long_piece_vocab.py.  v19 keeps the wide Viterbi and runs its rows of
pieces past 16 bytes (two-block hash, the pool's tail compare); v32 and v64 switch it off (every
17..48-byte word a long item) and run k_unigram_long<32> / <64>.  The tail compare's reject side
only runs for a string whose hash names the slot a piece sits in: the generator's collisions()
searches such strings (first and second probed slot), see test_v19_slot_collisions.  v19 has 48
new plain pieces, a guess at "enough that both cuckoo slots are used" -- nobody has computed the
slot each piece lands in -- and the retry after a header match in *both* slots is reached by no
case here: it stays unpinned.
"""
import json
import os
import random

import numpy as np
import pytest

import make_t5_long_piece_vocab as lp
import oracle_lib
import uni_census
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher
from test_gpu_span import run, torch  # noqa: F401  (the module-scoped torch fixture)

pytestmark = pytest.mark.gpu
S = 2048
ARENA_MAX = 64 << 10
K = uni_census.constants()
CH = K["CHUNK"]
MED_SLOTS = K["ARENA"] // K["UNI_WMAX"]


class Dev:
    """One vocabulary: its DeviceBatcher, oracle tokenizer, census and filler material."""

    def __init__(self, path):
        with open(path, encoding="utf-8") as f:
            vocab = json.load(f)["model"]["vocab"]
        self.census = uni_census.Census(vocab)
        self.tok = oracle_lib.T5Tok(path)
        self.db = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=64, sequence_length=S, min_ids=0,
                                tokenizer=path)
        # printable-ASCII plain pieces of the proxy (no "<" / ">": no added token can form)
        self.parts = [p for p, _ in vocab[3:32000] if not p.startswith("▁") and len(p) <= 16 and
                      all(0x21 <= ord(c) <= 0x7E and c not in "<>" for c in p)]

    def cat(self, rng, n):
        """n bytes of concatenated proxy pieces: a simple word with a realistic lattice."""
        s = ""
        while len(s) < n:
            s += rng.choice(self.parts)
        return s[:n]

    def misses(self, rng, lens):
        """Words of lower-case letters that no word-table rule produces."""
        out = []
        for n in lens:
            while True:
                w = "".join(rng.choice("bcdfghjklmnpqrstvwxz") for _ in range(n))
                if self.census.clear_miss(w) and w not in out:
                    out.append(w)
                    break
        return out

    def chunks(self, blobs):
        """The census of every 1 KiB chunk of the arena the blobs make, and the records' offsets."""
        offs = np.zeros(len(blobs) + 1, np.uint64)
        np.cumsum([len(b) for b in blobs], out=offs[1:])
        assert int(offs[-1]) <= ARENA_MAX
        return self.census.chunks(np.frombuffer(b"".join(blobs), np.uint8), offs), offs

    def check(self, torch, blobs):
        """Device ids of every record == the oracle's; returns the oracle's ids per record."""
        assert sum(map(len, blobs)) <= ARENA_MAX
        res = run(torch, self.db, blobs)
        assert res.tokenize_errors() == 0
        ids, am, _, _ = res.planes()
        per = res.record_rows()
        want, g = [], 0
        for r, b in enumerate(blobs):
            seq = []
            for _ in range(int(per[r])):
                z = int((am[g] == 0).sum())
                seq += ids[g, :S if z == 0 else z].tolist()
                g += 1
            w = self.tok.encode(b)
            assert seq[1:-1] == w, f"record {r}: {bytes(b[:80])!r}"  # [</s>] ... [</s>]
            want.append(w)
        return want


def rec(words, fill="the", last=None):
    """The words joined by single spaces in a record of a whole number of chunks, padded with
    in-vocabulary filler words and spaces; `last`: a word that ends the record."""
    t = (words if isinstance(words, bytes) else " ".join(words).encode())
    tail = b"" if last is None else b" " + last.encode()
    size = -(-max(len(t) + len(tail), 1) // CH) * CH
    f = b" " + fill.encode()
    while size - len(t) - len(tail) >= len(f):
        t += f
    return t + b" " * (size - len(t) - len(tail)) + tail


def fit_lens(n, lo, hi, room=CH):
    """n word lengths cycling lo..hi, the longest shortened until n words and spaces fit."""
    lens = [lo + i % (hi - lo + 1) for i in range(n)]
    while sum(lens) + n > room:
        lens[lens.index(max(lens))] -= 1
    assert min(lens) >= lo
    return lens


@pytest.fixture(scope="module")
def proxy(native_lib):
    return Dev(native.T5_PROXY_TOKENIZER)


def _variant(tmp_path_factory, name):
    path = os.path.join(str(tmp_path_factory.mktemp("t5_" + name)), "tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(lp.build(name), f, ensure_ascii=False)
    d = Dev(path)
    d.name = name
    d.plan = lp.plan(name)
    d.new = set(lp.new_ids(name).values())
    return d


@pytest.fixture(scope="module")
def v19(native_lib, tmp_path_factory):
    return _variant(tmp_path_factory, "v19")


@pytest.fixture(scope="module")
def v32(native_lib, tmp_path_factory):
    return _variant(tmp_path_factory, "v32")


@pytest.fixture(scope="module")
def v64(native_lib, tmp_path_factory):
    return _variant(tmp_path_factory, "v64")


# ---- narrow job capacity (proxy) ---------------------------------------------------------
# k_unigram_chunks' `new_job` lambda (tokenize_unigram.hip): the job past UNI_VPC of a chunk is
# refused and its word becomes a long item (the `if (!done)` branch of the per-piece loop).

def test_narrow_job_capacity(torch, proxy):
    rng = random.Random(88)
    counts = [K["UNI_VPC"] - 1, K["UNI_VPC"], K["UNI_VPC"] + 1, 120, 170]
    blobs = [rec(proxy.misses(rng, fit_lens(n, 4, 9))) for n in counts]
    # UNI_VPC + 1 misses with the odd one out at either end of the chunk (lane order decides who loses)
    m = proxy.misses(rng, fit_lens(K["UNI_VPC"] + 1, 4, 9, CH - 200))
    blobs.append(rec(m[:-1], last=m[-1]))
    blobs.append(rec([m[0]] + ["the"] * 40 + m[1:]))
    cs, offs = proxy.chunks(blobs)
    assert all(len(b) == CH for b in blobs)
    assert [c["narrow"] for c in cs] == counts + [K["UNI_VPC"] + 1] * 2
    assert [c["narrow"] <= K["UNI_VPC"] for c in cs] == [True, True, False, False, False, False, False]
    assert all(c["wide"] == c["medium"] == c["long"] == 0 and c["units"] == c["narrow"] for c in cs)
    assert blobs[5].endswith(m[-1].encode()) and blobs[6].startswith(m[0].encode())
    proxy.check(torch, blobs)


# ---- wide jobs and payload units (proxy) -------------------------------------------------
# The `word_len` lambda and `kind[u] == 4` of k_unigram_chunks, the payload-unit check of
# `new_job`, k_unigram_viterbi<true>: its passes of at most PFX_JOBS jobs and its longest-first
# order (the counting sort over `__ballot(keyv[g] == k)`).

def test_wide_boundary_lengths(torch, proxy):
    rng = random.Random(1648)
    WM, VM = K["UNI_WMAX"], K["UNI_VMAX"]
    lens = [WM, WM + 1, VM, VM + 1]
    words = [proxy.cat(rng, n) for n in lens] + proxy.misses(rng, [WM])
    blobs = [rec([w]) for w in words]
    # a 17..48-byte word with one control byte is not simple: a long item
    ctl = [proxy.cat(rng, 10) + c + proxy.cat(rng, n - 11) for n in (WM + 1, 30, VM) for c in ("\x7f", "\x1f")]
    blobs += [rec([w]) for w in ctl]
    cs, _ = proxy.chunks(blobs)
    assert [(c["wide"], c["long"]) for c in cs[:4]] == [(0, 0), (1, 0), (1, 0), (0, 1)]
    assert cs[4]["narrow"] == 1 and cs[1]["units"] == 2 and cs[2]["units"] == 3
    assert all(c["long"] == 1 and c["wide"] == c["medium"] == 0 for c in cs[5:]) and len(cs) == 11
    proxy.check(torch, blobs)


@pytest.mark.parametrize("length,n,fits", [(17, 43, True), (17, 44, True), (17, 45, False),
                                           (33, 29, True), (33, 30, False)])
def test_wide_payload_units(torch, proxy, length, n, fits):
    rng = random.Random(length * 100 + n)
    blobs = [rec([proxy.cat(rng, length) for _ in range(n)])]
    cs, _ = proxy.chunks(blobs)
    assert len(blobs[0]) == CH and cs[0]["wide"] == n and cs[0]["long"] == 0
    assert cs[0]["units"] == n * ((length + 15) // 16)
    assert (cs[0]["units"] <= K["UNI_VPC"]) == fits  # 86, 88 | 90; 87 | 90 units against 88
    proxy.check(torch, blobs)


@pytest.mark.parametrize("narrow,wide,fits", [(58, 15, True), (60, 15, False)])
def test_narrow_and_wide_share_the_unit_budget(torch, proxy, narrow, wide, fits):
    rng = random.Random(narrow)
    words = proxy.misses(rng, [4 + i % 3 for i in range(narrow)]) + [proxy.cat(rng, 17) for _ in range(wide)]
    rng.shuffle(words)
    blobs = [rec(words)]
    cs, _ = proxy.chunks(blobs)
    assert len(blobs[0]) == CH and (cs[0]["narrow"], cs[0]["wide"]) == (narrow, wide)
    assert cs[0]["narrow"] + cs[0]["wide"] <= K["UNI_VPC"]          # the jobs fit either way
    assert cs[0]["units"] == narrow + 2 * wide and (cs[0]["units"] <= K["UNI_VPC"]) == fits
    proxy.check(torch, blobs)


def test_wide_pass_edges_and_sort(torch, proxy):
    """1, PFX_JOBS, PFX_JOBS + 1, 2 PFX_JOBS, 2 PFX_JOBS + 1 wide jobs a chunk; then chunks whose
    wide words are all of one length, and of all-different lengths (the longest-first order is a
    counting sort over ballots)."""
    rng = random.Random(6)
    P = K["PFX_JOBS"]
    counts = [1, P, P + 1, 2 * P, 2 * P + 1]
    blobs = [rec([proxy.cat(rng, rng.randint(17, 48)) for _ in range(n)]) for n in counts]
    blobs.append(rec([proxy.cat(rng, 20) for _ in range(12)]))
    diff = list(range(17, 41))
    rng.shuffle(diff)
    blobs.append(rec([proxy.cat(rng, n) for n in diff]))
    cs, _ = proxy.chunks(blobs)
    assert [c["wide"] for c in cs] == counts + [12, 24]
    assert all(c["units"] <= K["UNI_VPC"] and c["long"] == 0 for c in cs)
    assert set(cs[5]["wide_lens"]) == {20} and sorted(cs[6]["wide_lens"]) == list(range(17, 41))
    proxy.check(torch, blobs)


# ---- medium words (proxy) ----------------------------------------------------------------
# k_unigram_chunks: the medium queue (`kind[u] == 2`, `s_med`, MED_CAP), the arena slots of the
# medium pass (`a + UNI_WMAX <= ARENA`), its normalize_span + split into `nvp` Viterbi pieces,
# `nvp == 0`, and a normalization past UNI_WMAX (normalize_span's `put` refuses: a long item).

MEDIUM = ["é", "naïve", "Zürich", "ﬁ", "½", "…", "㎏", "Ａ"]


@pytest.mark.parametrize("n,fits_slots,fits_queue", [(47, True, True), (48, True, True), (49, False, True),
                                                     (127, False, True), (128, False, True),
                                                     (129, False, False), (300, False, False)])
def test_medium_word_capacity(torch, proxy, n, fits_slots, fits_queue):
    words = [MEDIUM[i % len(MEDIUM)] for i in range(n)] if n <= 150 else ["é", "½"] * (n // 2)
    blobs = [rec(words)]
    cs, _ = proxy.chunks(blobs)
    assert len(blobs[0]) == CH and cs[0]["medium"] == n and cs[0]["long"] == 0 and cs[0]["narrow"] == 0
    # which side of the arena's slots and of the medium queue
    assert (cs[0]["medium"] <= MED_SLOTS) == fits_slots      # the arena's ARENA / UNI_WMAX slots
    assert (cs[0]["medium"] <= K["MED_CAP"]) == fits_queue   # the medium queue
    proxy.check(torch, blobs)


def test_medium_word_normalizations(torch, proxy):
    norm = proxy.tok.normalize
    gone, grows, splits = "\u200b", "\ufdfa", ["a\u3000b", "x\u00a0y", "\u00e9\u3000\u00e9\u00a0\u00e9"]
    assert norm(gone).strip() == ""                                   # nothing left: nvp == 0
    assert len(grows.encode()) <= K["UNI_WMAX"] < len(norm(grows).encode())  # past the slot: a long item
    assert all(len(w.encode()) <= K["UNI_WMAX"] and len(norm(w).split()) > 1 for w in splits)  # nvp > 1
    blobs = [rec([gone] * 20), rec([grows] * 20), rec(splits * 10),
             rec([gone, "the", grows, "é"] + splits)]
    cs, _ = proxy.chunks(blobs)
    assert [c["medium"] for c in cs] == [20, 20, 30, 6] and all(c["long"] == 0 for c in cs)
    proxy.check(torch, blobs)


# ---- id-dense chunks (proxy) -------------------------------------------------------------
# A medium word whose id bound exceeds its stage room (`bound > stage_room(pi)`) and a word
# table miss without room for its ids (`len + 1 <= room`) become long items; the chunk's entry
# count is as large as these inputs make it (1,023 and 1,024 of the 1,152 a chunk can list:
# common.hpp asserts that STAGE fits the packed scan's 11-bit field).  A 1 KiB chunk of k-byte words separated by
# single spaces cannot hold more ids than bytes: the oracle gives 1,023 ids for "½ " chunks,
# 512 for "㌀ " and for single letters, 256 for "… " -- so those four assert their own density,
# and the chunk of one-byte records (two ids a byte) is the one above 1,024.

@pytest.mark.parametrize("unit,ids_per_word", [("½", 3), ("…", 1), ("㌀", 2), ("letters", 1)])
def test_id_dense_chunks(torch, proxy, unit, ids_per_word):
    if unit == "letters":
        text = " ".join("abcdefghijklmnopqrstuvwxyz"[i % 26] for i in range(CH // 2)) + " "
    else:
        text = (unit + " ") * (CH // len((unit + " ").encode()))
    blobs = [rec(text.encode(), fill=unit if unit != "letters" else "a")] * 3
    n_words = len(text.split())
    cs, _ = proxy.chunks(blobs)
    assert all(len(b) == CH for b in blobs)
    if unit == "letters":
        assert cs[0]["hits"] + cs[0]["narrow"] == n_words == CH // 2
    else:
        assert cs[0]["medium"] == n_words > K["MED_CAP"]  # past the medium queue: long items too
        chars = len(proxy.tok.normalize(unit))
        room = len((unit + " ").encode())
        assert (chars + 1 > room) == {"½": True, "…": False, "㌀": True}[unit]  # `bound > stage_room`
    want = proxy.check(torch, blobs)
    assert all(len(w) - 1 == n_words * ids_per_word for w in want)  # (- the template's </s>)


def test_id_dense_one_byte_records(torch, proxy):
    """1,024 records of one byte ";" ("▁;" is no piece): "▁" and ";", two ids a byte -- 2,048 ids
    from one chunk, every word a miss with stage room for one id only (`len + 1 <= room` fails), so a long item."""
    assert not proxy.census.in_word_table(";") and len(proxy.tok.encode(";")) == 2 + 1
    blobs = [b";"] * CH
    cs, _ = proxy.chunks(blobs)
    assert len(cs) == 1 and cs[0]["narrow"] == CH and all(len(b) == 1 for b in blobs)  # room 1 < 2 ids
    want = proxy.check(torch, blobs)
    assert sum(len(w) - 1 for w in want) == 2 * CH > 1024


# ---- long-item stages (proxy; v32 / v64 below) --------------------------------------------
# k_unigram_long<KMAX, LONG_NORM1> -> <KMAX, LONG_NORM> -> k_unigram_huge: an item moves to the
# next stage's list when its normalized text exceeds NORM (`nl < 0`); printable ASCII words that
# fit the stage are copied without normalizing (`ascii`).

STAGE_LENS = [K["LONG_NORM1"] - 1, K["LONG_NORM1"], K["LONG_NORM1"] + 1, K["LONG_NORM"] - 1, K["LONG_NORM"],
              K["LONG_NORM"] + 1, 600, 5000]


def stage_words(dev, rng, n):
    """Words of n normalized bytes: printable ASCII, one that shrinks ("ﬁ" -> "fi"), one that
    grows ("½" -> "1⁄2"); the lengths are the oracle normalizer's."""
    shrink = "ﬁ" * (n // 2) + "x" * (n % 2)
    grow = "½" * (n // 5) + "x" * (n % 5)
    out = [dev.cat(rng, n), shrink, grow]
    for w in out:
        assert len(dev.tok.normalize(w).encode()) == n
    assert len(shrink.encode()) > n > len(grow.encode()) or n < 5
    return out


def check_stages(torch, dev, seed):
    rng = random.Random(seed)
    blobs = [w.encode() for n in STAGE_LENS for w in stage_words(dev, rng, n)]
    cs, offs = dev.chunks(blobs)
    assert sum(c["long"] for c in cs) == len(blobs) == 24  # one long item a record, nothing else
    assert all(c["narrow"] == c["wide"] == c["medium"] == c["hits"] == 0 for c in cs)
    assert [n <= K["LONG_NORM1"] for n in STAGE_LENS] == [True, True] + [False] * 6
    assert [n <= K["LONG_NORM"] for n in STAGE_LENS] == [True] * 5 + [False] * 3
    return dev.check(torch, blobs)


def test_long_item_stages(torch, proxy):
    check_stages(torch, proxy, 512)


def test_long_raw_staging_edge(torch, proxy):
    """Printable ASCII words of 1,006..1,024 bytes at arena positions p with p % 16 in {0, 1, 15}.
    k_unigram_long stages LONG_RAW raw bytes from (p - 1) & ~15 in LDS and its `byte` lambda reads
    past them from global text: these words end inside, at the end of, and past the staging, so
    word-end scan and normalize_span cross from one source to the other.  (They are longer than
    either stage's NORM, so the `ascii` copy is not taken and `p - pa + wl <= LONG_RAW` never
    decides anything here; the items end in k_unigram_huge.)"""
    rng = random.Random(1006)
    blobs, pos = [], 0
    for n in range(1006, 1025):
        for a in (0, 1, 15):
            pad = (a - pos) % 16
            blobs.append(b" " * pad + proxy.cat(rng, n).encode())
            assert (pos + pad) % 16 == a
            pos += len(blobs[-1])
    cs, offs = proxy.chunks(blobs)
    assert pos <= ARENA_MAX and sum(c["long"] for c in cs) == len(blobs) == 57
    # the word's last byte on both sides of the staging's end
    sides = {(((int(o) + len(b) - len(b.lstrip())) - 1) % 16 + 1 + len(b.strip()) <= K["LONG_RAW"])
             for o, b in zip(offs, blobs)}
    assert sides == {True, False}
    proxy.check(torch, blobs)


def test_words_running_past_the_window(torch, proxy):
    """Words of 25..48 bytes starting in a chunk's last 48 bytes: the one whose end the window still
    shows is a wide job, one byte further its length is unknown (word_len returns 0: a long item).
    (The window shows CHUNK + HALO_R - 8 bytes from the chunk's start, so a word of 17..24 bytes
    that starts in the chunk always ends in sight: the 17-byte word on the chunk's last byte.)"""
    rng = random.Random(48)
    lim = CH + K["HALO_R"] - 8
    blobs, want_kind = [], []
    cases = [(K["UNI_WMAX"] + 1, CH + K["UNI_WMAX"], "wide")]
    cases += [(L, end, kind) for L in (25, 32, 40, K["UNI_VMAX"])
              for end, kind in ((lim - 1, "wide"), (lim, "long"), (lim + 7, "long"))]
    for L, end, kind in cases:
        start = end - L
        if not CH - K["UNI_VMAX"] <= start < CH:
            continue
        head = rec(["the"] * 50)[:start - 1] + b" "
        blobs.append(rec(head + proxy.cat(rng, L).encode() + b" "))
        want_kind.append(kind)
    cs, _ = proxy.chunks(blobs)
    assert all(len(b) == 2 * CH for b in blobs) and len(blobs) == 12 and want_kind.count("wide") == 5
    assert [("wide" if c["wide"] else "long") for c in cs[::2]] == want_kind
    assert all(c["wide"] + c["long"] == 1 for c in cs[::2]) and all(c["wide"] + c["long"] == 0 for c in cs[1::2])
    proxy.check(torch, blobs)


# ---- v19: the wide Viterbi's rows of pieces past 16 bytes ---------------------------------
# k_unigram_viterbi<true>: the `n > 16` rows -- the two-block hash and `meta[u] |= cur_ps << 12`,
# the compare of the bytes past 16 against `T.vpool` -- and the prefix bound (`s_pl`, `T.upfx`).
# What each case can and cannot notice:
#   * the pieces themselves pin the accept side of the tail compare (a wrong pool or payload
#     index drops the long piece and changes ids), the two-block hash and the bound's rise;
#   * pair partners and near misses hash over all their bytes, so they name two other slots and
#     are rejected by the header before the tail compare is asked: they pin nothing about it;
#   * test_v19_slot_collisions has strings whose hash names a slot the piece may sit in, the
#     reject side of the compare, for the first and for the second probed slot;
#   * the retry for a header match in both slots (`id < 0 && m1 && slot_match(P[u].a2, ...)`)
#     needs two pieces with the same length and first 16 bytes in the two slots of one hash;
#     no case builds that, it stays unpinned.

def embed(dev, rng, piece, off, total):
    return dev.cat(rng, off) + piece + dev.cat(rng, total - off - len(piece))


def near_misses(p):
    """p with byte 17, 18 or 19 changed (those it has)."""
    return [p[:i] + ("#" if p[i] != "#" else "%") + p[i + 1:] for i in range(16, len(p))]


def pack_words(words, per_chunk):
    return [rec(words[i:i + per_chunk]) for i in range(0, len(words), per_chunk)]


def test_v19_vocabulary_keeps_the_wide_path(v19):
    c = v19.census
    assert c.maxlen_first == 19 and c.maxlen_meta == 16 and c.wide_ok
    assert c.maxlen_first > K["UNI_WMAX"] and c.maxlen_first < K["UNI_VRING"]


def test_v19_pieces_at_every_offset(torch, v19):
    """Every new plain piece at every offset 0 .. 48 - len of a 48-byte word: wide jobs, 20 a chunk
    (60 payload units), two arenas."""
    rng = random.Random(19)
    VM = K["UNI_VMAX"]
    pieces = v19.plan["plain"]
    words = [embed(v19, rng, p, off, VM) for p in pieces for off in range(VM - len(p) + 1)]
    used = 0
    for i in range(0, len(words), 1200):
        blobs = pack_words(words[i:i + 1200], 20)
        cs, _ = v19.chunks(blobs)
        assert all(len(b) == CH for b in blobs)
        assert sum(c["wide"] for c in cs) == len(words[i:i + 1200]) and all(c["long"] == 0 for c in cs)
        assert all(c["units"] <= K["UNI_VPC"] and c["wide"] <= K["UNI_VPC"] for c in cs)
        used += sum(1 for w in v19.check(torch, blobs) for x in w if x in v19.new)
    assert used > 0  # the oracle's output holds the new ids


def test_v19_pieces_alone_pairs_and_near_misses(torch, v19):
    """Every new piece as a word of its own (17..19 bytes: wide jobs; "▁" payloads of 14..16 bytes:
    narrow jobs or word-table hits), both members of every pair next to each other, and near
    misses differing from a piece at byte 17, 18 or 19.  (Partners and near misses hash to other
    slots than the piece, so the header rejects them: see test_v19_slot_collisions for the tail
    compare's reject side.)"""
    plain, meta = v19.plan["plain"], v19.plan["meta"]
    words = list(plain)
    for a, b in v19.plan["pairs"]:
        words += [a, b, b, a]
    nm = [w for p in plain for w in near_misses(p)]
    words += nm
    blobs = pack_words(words, 40) + pack_words(meta, 40)
    cs, _ = v19.chunks(blobs)
    assert sum(c["wide"] for c in cs) == len(words) and all(c["long"] == c["medium"] == 0 for c in cs)
    assert all(c["units"] <= K["UNI_VPC"] for c in cs)
    assert sum(c["hits"] for c in cs[-1:]) >= len(meta)  # "▁" + payload is a piece: a word-table hit
    assert len(nm) == sum(len(p) - 16 for p in plain)
    want = v19.check(torch, blobs)
    assert v19.new & {x for w in want for x in w}  # the oracle's output holds the new ids


def collision_words(dev, name, rng, total):
    """The generator's collision strings: alone, and at an offset inside a word of `total` bytes."""
    col = lp.collisions(name)
    assert col and all(len(s) == len(p) and s[:-3] == p[:-3] and s != p for p, s, _, _ in col)
    # equal slot indices, under the same hash the table builder and the kernels use
    assert all(lp.piece_slots(s.encode())[k - 1] == lp.piece_slots(p.encode())[j - 1] for p, s, k, j in col)
    # whichever of its two slots a piece was given, a string's first (k = 1) and a string's
    # second (k = 2) probed slot meet it: pieces with all four (k, j) kinds exist
    kinds = {}
    for p, _, k, j in col:
        kinds.setdefault(p, set()).add((k, j))
    assert sum(1 for v in kinds.values() if len(v) == 4) >= 8
    strings = [s for _, s, _, _ in col]
    return strings, [embed(dev, rng, s, rng.randint(1, total - len(s)), total) for s in strings]


def test_v19_slot_collisions(torch, v19):
    """The reject side of the tail compare in k_unigram_viterbi<true>'s `n > 16` rows and in
    k_unigram_long<20>'s `gen[u] == -3` probes.  Each string has a 19-byte piece's length and
    first 16 bytes, another tail, and a hash that names one of the piece's two slots as its first
    or as its second slot (tests/golden/make_t5_long_piece_vocab.py: collisions): where the piece
    sits there, the header matches and only the compare against the pool rejects the candidate.
    A kernel that accepted on the header alone would emit the piece's id (score -8: it wins)."""
    rng = random.Random(1918)
    alone, inside = collision_words(v19, "v19", rng, K["UNI_VMAX"])
    _, long60 = collision_words(v19, "v19", rng, 60)
    ids = lp.new_ids("v19")
    for p, s, _, _ in lp.collisions("v19"):
        assert ids[p] not in v19.tok.encode(s)  # the oracle does not see the piece in the string
    blobs = pack_words(alone, 40) + pack_words(inside, 20)
    n_wide = len(blobs)
    blobs += pack_words(long60, 16)
    cs, _ = v19.chunks(blobs)
    assert sum(c["wide"] for c in cs[:n_wide]) == len(alone) + len(inside)
    assert all(c["units"] <= K["UNI_VPC"] and c["long"] == 0 for c in cs[:n_wide])
    assert sum(c["long"] for c in cs[n_wide:]) == len(long60) and all(c["wide"] == 0 for c in cs[n_wide:])
    v19.check(torch, blobs)


def test_v19_long_and_non_simple_forms(torch, v19):
    """The same pieces in words of 60 bytes (past UNI_VMAX: long items, k_unigram_long<20> with
    pieces past 16 bytes: its `len <= 32` two-block probe, `gen[u] == -3`) and with an "é" appended (not simple: long
    items through the normalizer)."""
    rng = random.Random(60)
    plain = v19.plan["plain"]
    long60 = [v19.cat(rng, 60 - len(p)) + p for p in plain] + [p + v19.cat(rng, 60 - len(p)) for p in plain]
    accent = [p + "é" for p in plain] + [v19.cat(rng, 5) + p + "é" for p in plain]
    blobs = pack_words(long60, 16) + pack_words(accent, 30)
    cs, _ = v19.chunks(blobs)
    assert sum(c["long"] for c in cs) == len(long60) + len(accent)
    assert all(c["wide"] == c["narrow"] == c["medium"] == 0 for c in cs)
    want = v19.check(torch, blobs)
    assert v19.new & {x for w in want for x in w}


def test_v19_capacity_cases_again(torch, v19):
    """The proxy's wide unit and pass-edge cases with words made of the new pieces."""
    rng = random.Random(1919)
    plain = v19.plan["plain"]
    p17 = [p for p in plain if len(p) == 17]
    P = K["PFX_JOBS"]
    blobs = [rec([rng.choice(p17) for _ in range(n)]) for n in (43, 44, 45)]
    blobs += [rec([embed(v19, rng, rng.choice(plain), rng.randint(0, 14), 33) for _ in range(n)]) for n in (29, 30)]
    blobs += [rec([embed(v19, rng, rng.choice(plain), 3, rng.randint(24, 48)) for _ in range(n)])
              for n in (1, P, P + 1, 2 * P, 2 * P + 1)]
    cs, _ = v19.chunks(blobs)
    assert [c["wide"] for c in cs] == [43, 44, 45, 29, 30, 1, P, P + 1, 2 * P, 2 * P + 1]
    assert [c["units"] <= K["UNI_VPC"] for c in cs] == [True, True, False, True, False] + [True] * 5
    v19.check(torch, blobs)


# ---- v32 / v64: the wide Viterbi off, k_unigram_long<32> / <64> ----------------------------
# `wide_ok` false in k_unigram_chunks: every 17..48-byte word is a long item; k_unigram_long's
# two-block probes of 17..32-byte candidates (`gen[u] == -3`) and probe_acc for longer ones;
# launch_unigram_chunks picks the instantiation from maxlen_meta / maxlen_first
# (UNI_LONG_STAGES).  v32's collision strings (make_t5_long_piece_vocab.collisions) reach the
# reject side of the `gen[u] == -3` tail compare; probe_acc's, for pieces past 32 bytes, is
# reached by no case here.

def check_long_variant(torch, dev, lo, hi, meta_lo, meta_hi):
    c = dev.census
    assert (c.maxlen_first, c.maxlen_meta) == (hi, meta_hi) and not c.wide_ok
    rng = random.Random(hi)
    plain, meta = dev.plan["plain"], dev.plan["meta"]
    WM, VM = K["UNI_WMAX"], K["UNI_VMAX"]
    # boundary lengths, from the pieces (cut or embedded)
    bl = [rng.choice(plain)[:WM], (rng.choice(plain) + dev.cat(rng, WM))[:WM + 1],
          embed(dev, rng, plain[0], 0, max(VM, len(plain[0]))), embed(dev, rng, plain[0], 1, max(VM, len(plain[0])) + 1)]
    blobs = [rec([w]) for w in bl]
    cs, _ = dev.chunks(blobs)
    assert all(x["wide"] == 0 for x in cs) and [x["long"] for x in cs] == [0, 1, 1, 1]
    dev.check(torch, blobs)
    # the pieces alone, embedded, as near misses, with an accent, and the "▁" payloads as word starts
    words = list(plain) + list(meta)
    words += [embed(dev, rng, p, rng.randint(1, 9), len(p) + rng.randint(10, 20)) for p in plain]
    words += [m + dev.cat(rng, rng.randint(1, 9)) for m in meta]
    words += [p[:-1] + ("#" if p[-1] != "#" else "%") for p in plain + meta]
    words += [p[:16] + ("#" if p[16] != "#" else "%") + p[17:] for p in plain + meta]
    words += [p + "é" for p in plain]
    if dev.name == "v32":  # strings that name a piece's slot: the `gen[u] == -3` tail compare rejects
        alone, inside = collision_words(dev, "v32", rng, 60)
        words += alone + inside
    blobs = pack_words(words, 12)
    cs, _ = dev.chunks(blobs)
    assert all(x["wide"] == 0 for x in cs)  # wide_ok is false
    assert sum(x["long"] for x in cs) == len(words)
    want = dev.check(torch, blobs)
    assert dev.new & {x for w in want for x in w}  # the oracle's output holds the new ids
    # the long-item stages, words made of the pieces
    blobs = []
    for n in STAGE_LENS[:7]:
        w = ""
        while len(w) < n:
            w += rng.choice(plain)
        blobs += [w[:n].encode(), ("ﬁ" + w)[:n - 1].encode(), (rng.choice(meta) + w)[:n].encode()]
    cs, _ = dev.chunks(blobs)
    assert sum(x["long"] for x in cs) == len(blobs) and all(x["wide"] == 0 for x in cs)
    want = dev.check(torch, blobs)
    assert dev.new & {x for w in want for x in w}


def test_v32_long_items(torch, v32):
    check_long_variant(torch, v32, 20, 32, 17, 31)


def test_v64_long_items(torch, v64):
    check_long_variant(torch, v64, 33, 64, 32, 63)


def test_v32_v64_stage_forms(torch, v32, v64):
    """The proxy's stage-length words (ASCII, shrinking, growing) through <32> and <64>."""
    check_stages(torch, v32, 32)
    check_stages(torch, v64, 64)
