"""GPU parity of the word extents of the WordPiece chunk kernel's first probes
(tokenize_wordpiece.hip step 4, wp_extent.hpp): a word's length and fast flag come from two
per-chunk bitmaps (stop bytes, fast terminators) that every lane builds from its own 16 bytes, and
its bytes are lower-cased by one OR.

The texts are placed by byte offset: every generator asserts on the CPU that the bytes and the
record boundaries it is named for lie at the chunk offsets it wants.  Four arenas of 4-20 KiB --
arena i ends with a word of 15 + i letters -- and one above 64 chunks (the rows kernel then reads
the chunk lists themselves); every row is compared with the CPU oracle."""
import functools

import pytest

import oracle_lib

from test_gpu_parity import torch  # noqa: F401
from test_gpu_wordpiece_fixed_cost import CHUNK, MANY, UNK, Arena, check_rows, filler, word_ids

pytestmark = pytest.mark.gpu

# what may follow a word's run of letters: whitespace, punctuation, control bytes, a non-ASCII
# letter, non-ASCII whitespace (2- and 3-byte), non-ASCII punctuation, an added token, and (None)
# a record boundary
TERMS = (" ", ",", "\x01", "\x7f", "\u00e9", "\u00a0", "\u2003", "\u2014", "[MASK]", None)
WORDS = {3: "The", 5: "Their", 15: "Characteristics", 16: "Responsibilities", 17: "Telecommunication",
         18: "Telecommunications"}
assert all(len(w) == n and w.isascii() and w.isalpha() for n, w in WORDS.items())


def made_up(n):
    """n letters that are no word: several ids (or [UNK]) through the pending walk."""
    return (MANY * 4)[:n].upper()


def place(a, end_at, word, term):
    """`word` so that the byte behind it is chunk offset end_at % CHUNK, and `term` there."""
    start = (end_at - len(word)) % CHUNK
    a.goto(start)
    a.mark(start, word)
    if term is None:
        a.end(at=end_at % CHUNK)
        a.add("of ")
    else:
        a.mark(end_at % CHUNK, term)
        a.add(" of ")


def gen_edges(a, terms):
    """Each terminator with the word's end at a lane edge (15/16/17), at the bitmap words' edges
    (31/32/33, 63/64/65), at the chunk's end (1023, 1024) and in the right halo (1039, 1040)."""
    for t in terms:
        for k, (end_at, n) in enumerate(((1023, 16), (1024, 16), (1039, 16), (1040, 17))):
            if k < 3:
                for e, m in ((15 + k, 3), (31 + k, 5), (63 + k, 16)):
                    place(a, e, WORDS[m], t)
            place(a, end_at, WORDS[n] if k % 2 else made_up(n), t)


def gen_lengths(a, n):
    """A word of n letters (one in the vocabulary's reach, one made up) in front of each terminator."""
    for w in (WORDS[n], made_up(n), WORDS[n].lower()):
        for t in TERMS:
            a.add(w)
            if t is None:
                a.end()
            else:
                a.add(t)
                a.add("of " if t == " " else " of ")


def gen_misc(a, tok):
    # a record that starts at a chunk's first byte with a word
    a.goto(0, end="e")
    a.end(at=0)
    a.mark(0, "Unaffable of ")
    # a record boundary one byte into a run of letters
    a.add("the u")
    a.end()
    a.add("naffable of the U")
    a.end()
    a.add("NAFFABLE of ")
    # case and digits; the bytes next to the letter and digit ranges are pieces of their own
    a.add("THE The tHe ABC123xyz Z9 A@B a`b Z[z z{Z 0/9: the ")
    for s, n in (("A@B", 3), ("a`b", 3), ("Z[z", 3), ("z{Z", 3), ("0/9:", 4)):
        assert len(word_ids(tok, s)) == n and UNK not in word_ids(tok, s), s
    assert word_ids(tok, "THE") == word_ids(tok, "tHe") == word_ids(tok, "the")
    # an upper-case word that is no vocabulary entry: the pending walk, lower-cased
    w = (MANY + "qz").upper()
    assert len(word_ids(tok, w)) > 2 and UNK not in word_ids(tok, w) and word_ids(tok, w) == word_ids(tok, w.lower())
    a.add(w + " the " + w + ", " + w.capitalize() + " ")
    # a chunk that is one run of letters (over the 100-char cap: [UNK]); a piece start at every second byte
    a.goto(0)
    a.mark(0, "a" * CHUNK)
    a.add(" the ")
    assert word_ids(tok, "a" * CHUNK) == [UNK]
    a.goto(0)
    a.mark(0, "a," * (CHUNK // 2))
    a.add(" of the ")
    a.goto(0)
    a.mark(0, "Ab" * (CHUNK // 2 - 8) + " " * 16)


def gen_arena(a, tok, i):
    # (the terminators are of the classes they are named for)
    assert word_ids(tok, "the\u00a0of") == word_ids(tok, "the\u2003of") == word_ids(tok, "the of")
    assert len(word_ids(tok, "the\u2014of")) == 3 and len(word_ids(tok, "the[MASK]of")) == 3
    assert word_ids(tok, "the\x01of") == word_ids(tok, "the\x7fof") == word_ids(tok, "theof")
    assert len(word_ids(tok, "the\u00e9of")) == len(word_ids(tok, "theeof"))
    gen_edges(a, TERMS[i::4])
    if i == 3:
        gen_misc(a, tok)
    a.add(filler(a.rng, 40))
    gen_lengths(a, 15 + i)


@functools.lru_cache(maxsize=None)
def small_arena(i):
    tok = oracle_lib.Tok()
    a = Arena(40 + i)
    gen_arena(a, tok, i)
    last = WORDS[15 + i]
    a.add("the end is " + last)  # the arena ends inside the window of its last word
    records, arena = a.finish()
    assert arena.endswith(last.encode()) and 4 << 10 <= len(arena) <= 20 << 10, len(arena)
    return tuple(records)


@functools.lru_cache(maxsize=None)
def large_arena():
    """All four generators again, at other offsets, between filler records: more than 64 chunks."""
    tok = oracle_lib.Tok()
    a = Arena(77)
    for i in (2, 0, 3, 1, 3):
        a.add(filler(a.rng, a.rng.randint(300, 900)))
        a.end()
        gen_arena(a, tok, i)
        a.end()
    records, arena = a.finish()
    assert 64 * CHUNK < len(arena) <= 100 << 10, len(arena)
    return tuple(records)


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_small_arena_matches_oracle(torch, native_lib, oracle_tok, i):  # noqa: F811
    check_rows(torch, oracle_tok, small_arena(i))


def test_large_arena_matches_oracle(torch, native_lib, oracle_tok):  # noqa: F811
    """More than 64 chunks: no dense id array, the rows kernel reads the lists and rec_local."""
    check_rows(torch, oracle_tok, large_arena())
