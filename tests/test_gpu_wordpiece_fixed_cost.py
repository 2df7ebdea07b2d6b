"""GPU parity of the per-chunk fixed work of the WordPiece chunk kernel (tokenize_wordpiece.hip):
the id compaction from the stage slots' validity bitmap and the record boundaries' id offsets
(step 5, wp_pack.hpp), the state before the chunk (the look-back over the left halo) and the
non-ASCII lead bytes (step 2).

The texts are placed by byte offset: every generator asserts on the CPU that the bytes and the
record boundaries it is named for lie at the chunk offsets it wants.  Arenas are a few KiB, plus
one of 100-150 KiB (the rows kernel then reads the chunk lists and rec_local themselves); every
row is compared with the CPU oracle."""
import functools
import random

import numpy as np
import pytest

import oracle_lib
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_parity import framed_rows, run_device, torch  # noqa: F401

pytestmark = pytest.mark.gpu

CHUNK = 1024
HALO = 32
FILLER = "the of and to in a is that for it as was with be by on not he".split()
UNK = 100
MANY = "qzxjvk"  # repeated: a word of about one id a letter


def filler(rng, n, end=" "):
    """ASCII filler words, exactly n bytes, ending with `end`."""
    assert n >= len(end)
    s = ""
    while len(s) < n:
        s += rng.choice(FILLER) + " "
    return s[:n - len(end)] + end


def word_ids(tok, w):
    return tok.encode(w)[1:-1]  # (without the template's [CLS] / [SEP])


class Arena:
    """Records as bytes, built left to right with the arena offset known at every step."""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.records, self.cur, self.pos = [], b"", 0
        self.marks, self.bounds = [], []

    def add(self, s):
        b = s.encode("utf-8") if isinstance(s, str) else bytes(s)
        self.cur += b
        self.pos += len(b)

    def goto(self, at, end=" "):
        """Filler up to the next arena offset that is `at` into a chunk."""
        gap = (at - self.pos) % CHUNK
        if gap < len(end):
            gap += CHUNK
        self.add(filler(self.rng, gap, end))
        assert self.pos % CHUNK == at % CHUNK

    def mark(self, at, s):
        """`s` here, which must be chunk offset `at`; checked again on the finished arena."""
        b = s.encode("utf-8") if isinstance(s, str) else bytes(s)
        assert self.pos % CHUNK == at, (self.pos % CHUNK, at)
        self.marks.append((self.pos, b))
        self.add(b)

    def end(self, at=None):
        """A record boundary here (chunk offset `at` if given)."""
        if at is not None:
            assert self.pos % CHUNK == at, (self.pos % CHUNK, at)
        self.bounds.append(self.pos)
        self.records.append(self.cur)
        self.cur = b""

    def before_chunk(self, prefix, suffix, end=" "):
        """`prefix` ending exactly at a chunk's first byte, `suffix` from there."""
        pb = prefix.encode("utf-8") if isinstance(prefix, str) else bytes(prefix)
        self.goto(-len(pb) % CHUNK, end)
        self.mark(-len(pb) % CHUNK, pb)
        self.mark(0, suffix)

    def finish(self):
        if self.cur:
            self.end()
        arena = b"".join(self.records)
        offs = np.cumsum([0] + [len(r) for r in self.records])
        for p, b in self.marks:
            assert arena[p:p + len(b)] == b, p
        starts = set(int(o) for o in offs)
        for p in self.bounds:
            assert p in starts, p
        return self.records, arena


def chunk_of(arena, c):
    return arena[c * CHUNK:(c + 1) * CHUNK]


# ---- compaction and record boundaries ------------------------------------------------------
def gen_compaction(a, tok):
    props = {}
    a.add("the of and ")
    # a chunk of only whitespace
    a.goto(0)
    props["ws"] = a.pos // CHUNK
    a.mark(0, " " * 700 + "\n\t\r " * 100)
    a.add("and the ")
    # 1,024 one-byte pieces: more ids than the packing window holds, the direct store
    a.goto(1000)
    props["bang"] = a.pos // CHUNK + 1
    a.mark(1000, "!" * (24 + CHUNK + 10))
    a.add(" of ")
    # exactly 544 (the window's capacity) and 545 ids in a chunk
    a.goto(0)
    props["n544"] = a.pos // CHUNK
    a.mark(0, "!" * 544 + " " * (CHUNK - 544))
    a.mark(0, "!" * 545 + " " * (CHUNK - 545))
    # multi-id words from a chunk's last 16 bytes into the next: ids in the tail slots, through
    # the pending walk (<= 16 bytes), the lattice (> 16) and up to the tail's seventh lane
    for at, n in ((1018, 14), (1021, 42), (1023, 100), (1009, 60)):
        w = (MANY * 17)[:n]
        k = len(word_ids(tok, w))
        assert UNK not in word_ids(tok, w) and at + k > CHUNK, (at, k)
        a.goto(at)
        a.mark(at, w)
        a.add(" the ")
    assert 1023 + len(word_ids(tok, (MANY * 17)[:100])) - 1 >= CHUNK + 96  # lane 6 of the tail
    # a word that stages two pieces and then becomes [UNK]; what follows must not see them
    for head in ("unaffab", MANY + "qz"):
        w = head + "ꙮ"
        assert len(word_ids(tok, head)) >= 2 and UNK not in word_ids(tok, head)
        assert word_ids(tok, w) == [UNK]
        a.add(" " + w + " the " + w + "! " + w)
        a.end()
        a.add(w + " of ")
    # record boundaries: at a chunk's first byte
    a.goto(0)
    a.end(at=0)
    a.add("unaffable the ")
    # ... directly after a multi-id word (and the next record starts with one)
    assert len(word_ids(tok, "unaffable")) > 1
    a.add("of unaffable")
    a.end()
    a.add(MANY + " the")
    a.end()
    # ... inside a whitespace run
    a.add("the   \n ")
    a.end()
    a.add("  \t of the")
    # ... at a chunk's last byte
    a.goto(1023)
    a.end(at=1023)
    a.add("a unaffable the ")
    a.goto(1023, end="e")
    a.end(at=1023)
    a.add("unaffable ")
    # ... two empty records in a row
    a.end()
    a.end()
    a.end()
    a.add("the end of it")
    return props


def check_compaction(arena, props):
    assert chunk_of(arena, props["ws"]).strip() == b""
    assert chunk_of(arena, props["bang"]) == b"!" * CHUNK
    for d, n in ((0, 544), (1, 545)):
        c = chunk_of(arena, props["n544"] + d)
        assert c.count(b"!") == n and c.strip(b" ") == b"!" * n
        assert arena[props["n544"] * CHUNK - 1:props["n544"] * CHUNK] == b" "


# ---- the state before the chunk -----------------------------------------------------------------
def gen_lookback(a, tok):
    a.add("the of and ")
    cases = [
        ("tokeniz", "ation the "),                    # mid-word
        ("the ", "unaffable of "),                    # after a space
        ("the!", "unaffable of "),                    # after punctuation
        ("una" + "\x01" * (HALO + 8), "ffable of "),  # after a control run longer than the halo
        ("the [SEP]", "unaffable of "),               # directly after an added token
        ("the [MA", "SK] of "),                       # inside one
        ("the [MASK", "] of "),
        ("the [", "unaffable of "),                   # after a lone opener
        ("the [", "SEP] of "),
        ("the\u00a0", "unaffable of "),              # after NBSP, em-dash, e-acute, a combining mark
        ("the\u2014", "unaffable of "),
        ("caf\u00e9", "s of the "),
        ("cafe\u0301", "s of the "),
        ("the 中", "unaffable of "),
        ("un\U0001f600", "affable of "),
        ("the   \n\n", "unaffable of "),
    ]
    for prefix, suffix in cases:
        a.before_chunk(prefix, suffix)
    assert word_ids(tok, "una" + "\x01" * (HALO + 8) + "ffable") == word_ids(tok, "unaffable")
    assert word_ids(tok, "the [MASK] of")[1] == 103
    # a record start exactly at the chunk start, and one byte before it
    a.goto(0, end="e")
    a.end(at=0)
    a.add("unaffable of ")
    a.goto(1023, end="e")
    a.end(at=1023)
    a.add("unaffable of ")
    # ... with an added token and a non-ASCII char cut by them
    a.goto(1023, end=" ")
    a.end(at=1023)
    a.add("[SEP] of ")
    a.goto(1022, end=" ")
    a.mark(1022, "[")
    a.end(at=1023)
    a.add("SEP] of the ")


# ---- non-ASCII lead bytes ---------------------------------------------------------------------------
LEAD_CHARS = ("é", "—", "中", "\U0001f600", "\U00020000", "\U00010348")


def gen_leads(a, tok):
    a.add("the of and ")
    # an ISO char with an id of its own, one without (a supplementary-plane ideograph)
    assert word_ids(tok, "—") != [UNK] and word_ids(tok, "\U00020000") == [UNK]
    # a 2-, 3- and 4-byte char whose lead is byte 13, 14 or 15 of a lane's 16 ...
    for ch in LEAD_CHARS:
        for j in (13, 14, 15):
            a.add(filler(a.rng, (j - a.pos - 2) % 16 + 2))
            assert a.pos % 16 == j
            a.mark(a.pos % CHUNK, ch + "x " + ch + " un" + ch + "ble ")
    # ... and of the chunk's: the continuation bytes are in the right halo
    for ch in LEAD_CHARS[:2] + LEAD_CHARS[3:5]:
        for at in (1021, 1022, 1023):
            a.goto(at)
            a.mark(at, ch + ch + "x the ")
    # more than 64 leads in one chunk, and a chunk of nothing else
    a.goto(0)
    a.mark(0, "中" * 120 + " ")
    a.goto(1000)
    a.mark(1000, "é—" * 300 + " ")
    # a record boundary inside a multi-byte sequence, in a lane, across lanes and across chunks
    for at, head, tail in ((None, b"the \xe2\x80", b"\x94 of "), (16 * 7 + 15, b"\xe2", b"\x80\x94 of "),
                           (1022, b"\xe2\x80", b"\x94 of "), (1023, b"\xc3", b"\xa9s of "),
                           (1023, b"\xf0", b"\x9f\x98\x80 of "), (1021, b"\xf0\x9f\x98", b"\x80s of ")):
        if at is not None:
            a.goto(at)
            a.mark(at, head)
        else:
            a.add(head)
        a.end()
        a.add(tail)
    a.add("the end")


GENERATORS = {"compaction": gen_compaction, "lookback": gen_lookback, "leads": gen_leads}


@functools.lru_cache(maxsize=None)
def small_arena(name):
    tok = oracle_lib.Tok()
    a = Arena(len(name))
    props = GENERATORS[name](a, tok)
    records, arena = a.finish()
    if name == "compaction":
        check_compaction(arena, props)
        assert len(arena) % CHUNK != 0  # the last chunk is partial
        assert b"" in records
    return tuple(records)


@functools.lru_cache(maxsize=None)
def large_arena():
    """Every generator several times, at other offsets, between filler records: 100-150 KiB."""
    tok = oracle_lib.Tok()
    a = Arena(99)
    while a.pos < 100 << 10:
        for name in ("leads", "compaction", "lookback"):
            props = GENERATORS[name](a, tok)
            a.end()
            if name == "compaction":
                first = props
            a.add(filler(a.rng, a.rng.randint(300, 2500)))
            a.end()
    records, arena = a.finish()
    check_compaction(arena, first)
    assert 100 << 10 <= len(arena) <= 150 << 10, len(arena)
    assert len(arena) % CHUNK != 0
    return tuple(records)


def check_rows(torch, oracle_tok, records, S=512):  # noqa: F811
    records = list(records)
    db = DeviceBatcher(batch_size=16, sequence_length=S, mask_length=0, min_ids=0)
    ids = run_device(torch, db, records).planes()[0]
    want = framed_rows(oracle_tok, records, S)
    assert ids.shape == want.shape
    bad = np.nonzero((ids != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(want)} rows differ, first {bad[:5]}"
    db.close()


@pytest.mark.parametrize("name", ["compaction", "lookback", "leads"])
def test_small_arena_matches_oracle(torch, native_lib, oracle_tok, name):  # noqa: F811
    records = small_arena(name)
    assert sum(len(r) for r in records) < 64 * CHUNK
    check_rows(torch, oracle_tok, records)


def test_large_arena_matches_oracle(torch, native_lib, oracle_tok):  # noqa: F811
    """More than 64 chunks: no dense id array, the rows kernel reads the lists and rec_local."""
    check_rows(torch, oracle_tok, large_arena())
