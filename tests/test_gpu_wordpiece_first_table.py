"""GPU parity of the first probes of the WordPiece chunk kernel through the first-piece table
(tokenize_wordpiece.hip step 4a, wp_first.hpp): a fast word of at most 14 bytes is looked up in
a table of 16-byte slots that holds only the vocabulary's non-"##" pieces of that length, every
other word goes to the pending walk, and a round of first probes takes up to 256 pieces.

The texts are placed by byte offset: every generator asserts on the CPU that the bytes, the
record boundaries and the piece counts it is named for lie where it wants them.  One arena holds
every first piece of at most 17 bytes of the proxy vocabulary once as a word (every occupied slot
of the table is read on the device); the others are 10-80 KiB.  Every row is compared with the
CPU oracle."""
import functools
import json
import re

import pytest

import oracle_lib

from test_gpu_parity import torch  # noqa: F401
from test_gpu_wordpiece_fixed_cost import CHUNK, UNK, Arena, check_rows, chunk_of, filler, word_ids
from test_gpu_wordpiece_word_extent import place
from test_wp_first import TOKENIZER

pytestmark = pytest.mark.gpu

SLOT_BYTES = 14  # payload bytes of a slot of the first-piece table


@functools.lru_cache(maxsize=None)
def vocab():
    with open(TOKENIZER, encoding="utf-8") as f:
        return json.load(f)["model"]["vocab"]


def is_cont(p):
    return len(p) > 2 and p.startswith("##")


@functools.lru_cache(maxsize=None)
def first_pieces():
    """The non-"##" pieces in id order."""
    v = vocab()
    return tuple(p for p in sorted(v, key=v.get) if not is_cont(p))


def in_vocab(tok, w):
    ids = word_ids(tok, w)
    return len(ids) == 1 and ids != [UNK]


# ---- every first piece once ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_pieces_arena():
    pieces = [p for p in first_pieces() if len(p.encode()) <= 17]
    assert sum(len(p.encode()) <= SLOT_BYTES for p in pieces) > 20000
    assert any(len(p.encode()) == n for p in pieces for n in (15, 16, 17))
    records = [" ".join(pieces[i:i + 61]).encode() for i in range(0, len(pieces), 61)]
    assert 150 << 10 <= sum(len(r) for r in records) <= 260 << 10
    return tuple(records)


def test_every_first_piece_as_a_word(torch, native_lib, oracle_tok):  # noqa: F811
    check_rows(torch, oracle_tok, all_pieces_arena())


# ---- words of 13-17 bytes around the slot's 14 ------------------------------------------------------
def long_words(tok, n):
    """Two ASCII words of n letters that are pieces, and each with one letter changed so that it
    is none; one of each in upper and one in mixed case."""
    words = [p for p in first_pieces() if len(p) == n and p.isascii() and p.isalpha()][:2]
    assert len(words) == 2, n
    out = []
    for w in words:
        assert in_vocab(tok, w)
        off = next(x for x in (w[:k] + c + w[k + 1:] for k in (n // 2, n - 1, 0) for c in "qzx")
                   if x not in vocab())
        assert not in_vocab(tok, off)
        for x in (w, off):
            mixed = "".join(c.upper() if i % 2 else c for i, c in enumerate(x))
            out.append(mixed if len(out) % 3 else x.upper())  # upper, mixed, mixed, upper
            assert word_ids(tok, x.upper()) == word_ids(tok, mixed) == word_ids(tok, x)
    return out


# the byte behind the word: a lane's edges, the chunk's last bytes and first byte, the right halo
EDGES = (16, 17, 1023, 1024, 1025, 1039, 1040)


def gen_long(a, tok, n):
    a.add("the of and ")
    for w in long_words(tok, n):
        for end_at in EDGES:
            place(a, end_at, w, " ")
        place(a, 1024, w, None)  # a record start right after the word, at a chunk's first byte
        # ... and anywhere; the next record starts with the word
        a.add(w)
        a.end()
        a.add(w + " of ")
        # a record start inside the word: in a lane, and with the word across two chunks
        for k in (1, n // 2, n - 1):
            a.add("the " + w[:k])
            a.end()
            a.add(w[k:] + " of ")
        a.goto(CHUNK - n // 2)
        a.mark(CHUNK - n // 2, w[:n // 2])
        a.end(at=0)
        a.add(w[n // 2:] + " the ")


@functools.lru_cache(maxsize=None)
def long_arena(n):
    tok = oracle_lib.Tok()
    a = Arena(130 + n)
    gen_long(a, tok, n)
    a.add("the end")
    records, arena = a.finish()
    assert 10 << 10 <= len(arena) <= 80 << 10, len(arena)
    return tuple(records)


@pytest.mark.parametrize("n", [13, 14, 15, 16, 17])
def test_words_around_the_slot_length(torch, native_lib, oracle_tok, n):  # noqa: F811
    check_rows(torch, oracle_tok, long_arena(n))


# ---- "##" payloads and digits as whole words ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cont_arena():
    tok = oracle_lib.Tok()
    v = vocab()
    only = [p[2:] for p in sorted(v, key=v.get) if is_cont(p) and p[2:] not in v]
    assert len(only) > 1000
    assert any(x.isascii() and x.isalnum() and len(x) >= 6 for x in only)
    a = Arena(7)
    for i in range(0, len(only), 50):
        a.add(" ".join(only[i:i + 50]) + " the ")
        if i % 200 == 0:
            a.end()
    # digit words: pieces, none, and runs around the slot's 14 bytes
    digits = ["0", "7", "10", "1999", "2000", "1234", "98765", "31415926"] + ["1234567890123456789"[:n] for n in range(12, 19)]
    assert any(in_vocab(tok, d) for d in digits) and any(not in_vocab(tok, d) for d in digits)
    a.end()
    for d in digits:
        a.add(d + " " + d + ", x" + d + " " + d + "th ")
        for end_at in (16, 1024, 1040):
            place(a, end_at, d, " ")
    records, arena = a.finish()
    assert 10 << 10 <= len(arena) <= 80 << 10, len(arena)
    return tuple(records)


def test_cont_payloads_and_digit_words(torch, native_lib, oracle_tok):  # noqa: F811
    check_rows(torch, oracle_tok, cont_arena())


# ---- chunks of exactly K pieces ----------------------------------------------------------------------------
COUNTS = (127, 128, 129, 192, 193, 255, 256, 257, 512)
IN2 = ("of", "to", "in", "is", "it", "as", "be", "by", "on", "he")
OUT = ("qxz", "zqj", "xqz", "jqx")  # (and their first two letters)


def n_pieces(chunk):
    """Piece starts in a chunk of ASCII text that begins after whitespace: words and punctuation chars."""
    return len(re.findall(rb"[0-9A-Za-z]+|[!-/:-@\[-`{-~]", chunk))


def chunk_text(tok, K, form):
    """CHUNK bytes holding exactly K pieces.  form 0: every word is a piece of the vocabulary;
    1: every third piece is a word that is none (several ids through the pending walk, which the
    rounds of first probes then alternate with); 2: every piece is such a word."""
    one = [c for c in "abcdefghijklmnopqrstuvwxyz"]
    parts = []
    for i in range(K):
        if K > 257:  # one-byte pieces: a letter, a comma (a piece of its own, no probe), a word
            if form == 0:
                parts.append(one[i % 26] + " ")
            else:
                parts.append((one[i % 26], ",", OUT[i % 4][:2] + " ")[i % 3])
        elif form == 2 or (form == 1 and i % 3 == 2):
            parts.append(OUT[i % 4][:2 if form == 2 else 3] + " ")
        else:
            parts.append(IN2[i % 10] + " ")
    s = "".join(parts)
    assert len(s) <= CHUNK, (K, form, len(s))
    return s + " " * (CHUNK - len(s))


@functools.lru_cache(maxsize=None)
def counts_arena():
    tok = oracle_lib.Tok()
    for w in IN2 + tuple("abcdefghijklmnopqrstuvwxyz"):
        assert in_vocab(tok, w), w
    for w in OUT:
        for x in (w, w[:2]):
            assert not in_vocab(tok, x) and x not in vocab(), x
    a = Arena(512)
    a.add("the of and ")
    where = []
    for K in COUNTS:
        for form in (0, 1) + ((2,) if K in (256, 257) else ()):
            a.goto(0)
            where.append((a.pos // CHUNK, K))
            a.mark(0, chunk_text(tok, K, form))
            a.add("the of ")
            if form == 1:
                a.end()
    a.add("the end")
    records, arena = a.finish()
    for c, K in where:
        assert n_pieces(chunk_of(arena, c)) == K and arena[c * CHUNK - 1:c * CHUNK] == b" ", (c, K)
    assert 10 << 10 <= len(arena) <= 80 << 10, len(arena)
    return tuple(records)


def test_chunks_of_exact_piece_counts(torch, native_lib, oracle_tok):  # noqa: F811
    check_rows(torch, oracle_tok, counts_arena())
