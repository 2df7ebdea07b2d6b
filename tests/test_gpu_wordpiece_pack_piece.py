"""GPU parity of the WordPiece chunk kernel's id compaction (tokenize_wordpiece.hip step 5,
wp_pack.hpp) over chunks placed for its three ways out: a chunk without an exception bit gathers
its list through the piece descriptors; a chunk with exceptions (a word of more than one id) is
packed slot by slot in LDS and copied out; a chunk with exceptions and more ids than the packing
window holds stores straight to its slice.

Texts are placed by byte offset (the Arena of test_gpu_wordpiece_fixed_cost.py).  Every generator
first asserts on the CPU, from a census of the oracle's ids per word, that the chunks it names
hold exactly the pieces and the exceptions (words of more than one id) they are named for; then
every row is compared with the CPU oracle.  Arenas are a few KiB to 20 KiB, plus one of about
120 KiB (more than 64 chunks: the rows kernel reads the chunk lists and rec_local themselves).

A piece without an id cannot be made on the device: a word the oracle gives no id (a lone
combining mark, a control byte) consists of chars of the removed class, which start no piece,
and a char that does start one never normalizes to nothing (wp_pack.hpp).  So the no-id
exception bit is exercised by the host program of test_wp_pack_piece.py alone; here such words
stand in chunks of both kinds and must leave the lists around them alone."""
import functools
import re

import pytest

import oracle_lib

from test_gpu_parity import torch  # noqa: F401
from test_gpu_wordpiece_fixed_cost import CHUNK, FILLER, MANY, UNK, Arena, check_rows, word_ids

pytestmark = pytest.mark.gpu

WINDOW_IDS = 544  # ids the packing window holds (WIN / 2)
PLAIN_COUNTS = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513)
WORD_RE = re.compile(r"\w+|[^\w\s]")  # (no text here holds an underscore)


def census(tok, records):
    """chunk -> [pieces, words of more than one id, words of no id, ids], each word counted in
    the chunk of its first byte, from the oracle's ids per word."""
    out, base, cache = {}, 0, {}
    for rec in records:
        text = rec.decode("utf-8")
        at, done = 0, 0  # byte offset of text[:done]
        for m in WORD_RE.finditer(text):
            at += len(text[done:m.start()].encode("utf-8"))
            done = m.start()
            w = m.group()
            if w not in cache:
                cache[w] = len(word_ids(tok, w))
            c = out.setdefault((base + at) // CHUNK, [0, 0, 0, 0])
            c[0] += 1
            c[1] += cache[w] > 1
            c[2] += cache[w] == 0
            c[3] += cache[w]
        base += len(rec)
    return out


def filler(rng, n):
    """Whole filler words (one id each) and spaces, exactly n bytes, ending in a space."""
    s = ""
    while True:
        w = rng.choice(FILLER) + " "
        if len(s) + len(w) > n:
            return s + " " * (n - len(s))
        s += w


def plain_chunk(n):
    """1,024 bytes of exactly n one-id pieces, ending in whitespace: words while they fit (the
    first probes), '!' for the rest."""
    words = min(n, 200)
    s = "".join(FILLER[k % len(FILLER)] + " " for k in range(words)) + "!" * (n - words)
    assert len(s) < CHUNK
    return s + " " * (CHUNK - len(s))


class Named(Arena):
    """An Arena that remembers what its generator says about chunks: name -> (chunk, pieces or
    None, exceptions, no-id words), checked against the census of the finished arena."""

    def __init__(self, seed):
        super().__init__(seed)
        self.claims = []

    def claim(self, name, pieces=None, multi=0, noid=0, chunk=None):
        self.claims.append((name, self.pos // CHUNK if chunk is None else chunk, pieces, multi, noid))

    def goto(self, at):
        """Whole filler words up to the next arena offset that is `at` into a chunk."""
        self.add(filler(self.rng, (at - self.pos) % CHUNK or CHUNK))
        assert self.pos % CHUNK == at % CHUNK

    def fresh(self):
        """To the start of a chunk whose last byte before is whitespace."""
        if self.pos % CHUNK or (self.cur and not self.cur.endswith(b" ")):
            self.goto(0)
        return self.pos // CHUNK

    def rest(self):
        """Filler to the end of this chunk."""
        if self.pos % CHUNK:
            self.add(filler(self.rng, CHUNK - self.pos % CHUNK))


def finish(a, tok):
    records, arena = a.finish()
    got = census(tok, records)
    for name, c, pieces, multi, noid in a.claims:
        have = got.get(c, [0, 0, 0, 0])
        assert (have[1], have[2]) == (multi, noid), (name, c, have)
        if pieces is not None:
            assert have[0] == pieces, (name, c, have)
            if multi == 0:
                assert have[3] == pieces - noid, (name, c, have)
    return tuple(records), got


# ---- exception-free chunks ----------------------------------------------------------------------
def gen_plain(a, tok):
    assert all(len(word_ids(tok, w)) == 1 for w in FILLER + ["!"])
    a.add("the of and ")
    a.goto(0)
    for n in PLAIN_COUNTS:
        a.claim(f"plain{n}", pieces=n)
        a.mark(0, plain_chunk(n))
    # more ids than the packing window holds, none an exception: still the gather
    a.claim("plain_run", pieces=600)
    a.mark(0, "!" * 600 + " " * (CHUNK - 600))
    a.claim("plain_full", pieces=CHUNK)
    a.mark(0, "!" * CHUNK)
    a.add(" the end")


# ---- one multi-id word, alone in its chunk ------------------------------------------------------
def gen_places(a, tok):
    many = word_ids(tok, MANY)
    assert len(many) > 2 and UNK not in many
    a.add("the of and ")
    # as the chunk's first piece
    a.fresh()
    a.claim("first", multi=1)
    a.mark(0, MANY + " ")
    a.rest()
    # in lane 0 but not the first piece, and in lane 63 (slots 1010 ..)
    a.claim("lane0", multi=1)
    a.mark(0, "a " + MANY + " ")
    a.rest()
    a.claim("lane63", multi=1)
    a.goto(1010)
    a.mark(1010, MANY)
    assert 1010 + len(many) <= CHUNK
    a.add(" " * (CHUNK - a.pos % CHUNK))
    # as its last piece, whitespace behind it
    a.claim("last", multi=1)
    a.add(filler(a.rng, 700))
    a.add(MANY + " " * (CHUNK - a.pos % CHUNK - len(MANY)))
    # ending in the tail slots: more ids than bytes left in the chunk (the next chunk has none)
    for at, n in ((1018, 14), (1021, 42)):
        w = (MANY * 7)[:n]
        k = len(word_ids(tok, w))
        assert UNK not in word_ids(tok, w) and at + k > CHUNK, (at, k)
        a.fresh()
        a.claim(f"tail{at}", multi=1)
        a.goto(at)
        a.mark(at, w)
        a.claim(f"after_tail{at}", chunk=a.pos // CHUNK)
        a.add(" ")
        a.rest()
    # right before a record boundary (and the next record starts with one)
    a.claim("before_boundary", multi=1)
    a.add(filler(a.rng, 300) + MANY)
    a.end()
    a.add("the of ")
    a.rest()
    a.claim("after_boundary", multi=1)
    a.add(filler(a.rng, 200))
    a.end()
    a.add(MANY + " ")
    a.rest()
    # two in one 16-byte group
    for w in ("xj", "zq"):
        assert len(word_ids(tok, w)) == 2
    a.claim("two_in_group", multi=2)
    a.add(filler(a.rng, 16 * 9 + 2))
    a.mark(16 * 9 + 2, "xj zq ")
    a.rest()
    # a word that stages ids and then ends as [UNK]: no exception may be left behind
    w = "unaffabꙮ"
    assert len(word_ids(tok, "unaffab")) >= 2 and word_ids(tok, w) == [UNK]
    a.claim("unk_after_ids")
    a.add(filler(a.rng, 100) + w + " the " + w + "! ")
    a.rest()
    a.claim("unk_and_multi", multi=1)
    a.add(filler(a.rng, 100) + w + " " + MANY + " " + w + " ")
    a.rest()
    # words the oracle gives no id, in a chunk without and one with an exception
    gone = [s for s in ("\u0301", "\x01") if word_ids(tok, s) == []]
    assert gone
    a.claim("noid", noid=len(gone))
    a.add(filler(a.rng, 64) + "".join(s + " of " for s in gone))
    a.rest()
    a.claim("noid_and_multi", multi=1, noid=len(gone) + 1)
    a.add(filler(a.rng, 64) + "".join(s + " of " for s in gone) + MANY + " " + gone[0] + " ")
    a.rest()
    a.add("the end")


# ---- many exceptions, both sides of the window's capacity, chunks alternating ---------------------
def gen_dense(a, tok):
    k = len(word_ids(tok, MANY))
    a.add("the of and ")
    a.fresh()
    nb = WINDOW_IDS // k - 2  # packed in the window: at most the ids it holds
    a.claim("dense_window", pieces=nb, multi=nb)
    a.mark(0, (MANY + " ") * nb)
    a.add(" " * (CHUNK - a.pos % CHUNK))
    nc = CHUNK // (len(MANY) + 1)  # the straight path: more
    assert nc * k > WINDOW_IDS
    a.claim("dense_straight", pieces=nc, multi=nc)
    a.mark(0, (MANY + " ") * nc)
    a.add(" " * (CHUNK - a.pos % CHUNK))
    # a punctuation run and one exception: the straight path; exactly the window's ids: the window
    a.claim("run_and_multi", pieces=601, multi=1)
    a.mark(0, "!" * 600 + " " + MANY + " ")
    a.add(" " * (CHUNK - a.pos % CHUNK))
    for total in (WINDOW_IDS, WINDOW_IDS + 1):
        a.claim(f"total{total}", pieces=total - k + 1, multi=1)
        a.mark(0, "!" * (total - k) + " " + MANY + " ")
        a.add(" " * (CHUNK - a.pos % CHUNK))
    # exception and exception-free chunks alternating
    for j in range(6):
        a.claim(f"alt{j}", multi=j & 1)
        a.add(filler(a.rng, 400))
        if j & 1:
            a.add("unaffable ")
        a.rest()
    assert len(word_ids(tok, "unaffable")) > 1
    a.add("the end")


# ---- record boundaries -----------------------------------------------------------------------------
def gen_bounds(a, tok):
    a.add("the of and ")
    for multi in (0, 1):
        for at in (0, 15, 16, 1023):
            a.fresh()
            a.claim(f"bound{at}_{multi}", multi=multi)
            if at:
                a.goto(at)
            a.end(at=at)
            a.add((MANY if multi else "that") + " of ")
            a.rest()
    # every word a record, with and without exceptions; empty records
    a.claim("records", multi=3)
    for w in ("the", MANY, "of", "xj", "", "", "and", "unaffable", "it"):
        a.add(w)
        a.end()
    a.rest()
    a.add("the end")


GENERATORS = {"plain": gen_plain, "places": gen_places, "dense": gen_dense, "bounds": gen_bounds}


@functools.lru_cache(maxsize=None)
def small_arena(name, cased=False):
    tok = cased_oracle() if cased else oracle_lib.Tok()
    a = Named(len(name))
    GENERATORS[name](a, tok)
    records, _ = finish(a, tok)
    n = sum(len(r) for r in records)
    assert n % CHUNK != 0 and n < 24 * CHUNK  # the final chunk is short
    return records


def cased_oracle():
    import wp_cased_cases as W
    return W.oracle("cased")


@functools.lru_cache(maxsize=None)
def large_arena():
    tok = oracle_lib.Tok()
    a = Named(21)
    while a.pos < 100 << 10:
        for name in ("places", "dense", "bounds", "plain"):
            GENERATORS[name](a, tok)
            a.end()
            a.add(filler(a.rng, a.rng.randint(300, 2500)))
            a.end()
    records, _ = finish(a, tok)
    n = sum(len(r) for r in records)
    assert 100 << 10 <= n <= 160 << 10 and n % CHUNK != 0, n
    return records


@pytest.mark.parametrize("name", sorted(GENERATORS))
def test_small_arena_matches_oracle(torch, native_lib, oracle_tok, name):  # noqa: F811
    check_rows(torch, oracle_tok, small_arena(name))


@pytest.mark.parametrize("kind", ["plain", "exception", "empty"])
def test_one_chunk_arena_matches_oracle(torch, native_lib, oracle_tok, kind):  # noqa: F811
    """An arena of one chunk, shorter than 1,024 bytes."""
    a = Named(5)
    a.claim(kind, multi=int(kind == "exception"), pieces=0 if kind == "empty" else None)
    if kind == "empty":
        a.add("   \n ")
    else:
        a.add(filler(a.rng, 300) + ("unaffable" if kind == "exception" else "that"))
        a.end()
        a.add("of the")
    records, _ = finish(a, oracle_tok)
    assert sum(len(r) for r in records) < CHUNK
    check_rows(torch, oracle_tok, records)


def test_large_arena_matches_oracle(torch, native_lib, oracle_tok):  # noqa: F811
    check_rows(torch, oracle_tok, large_arena())


def test_cased_arena_matches_oracle(torch, native_lib):  # noqa: F811
    """The kernel's cased instantiation over the arena of placed multi-id words."""
    import wp_cased_cases as W
    import numpy as np
    from streaming_data_loader_amd.device import DeviceBatcher
    from test_gpu_parity import framed_rows, run_device
    tok = cased_oracle()
    records = list(small_arena("places", cased=True))
    want = framed_rows(tok, records, 512)
    db = DeviceBatcher(batch_size=16, sequence_length=512, mask_length=0, min_ids=0,
                       tokenizer=W.native.BERT_CASED_PROXY_TOKENIZER)
    ids = run_device(torch, db, records).planes()[0]
    assert ids.shape == want.shape
    bad = np.nonzero((ids != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(want)} rows differ, first {bad[:5]}"
    db.close()
