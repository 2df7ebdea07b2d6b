#!/usr/bin/env python3
"""t5 Unigram tokenizer.json variants whose piece scores tie (test infrastructure: the
fixtures of tests/test_t5_tied_scores.py and tests/test_gpu_unigram_ties.py).

The proxy asset has 32,100 practically distinct 17-digit scores, so two segmentations of a
word almost never have equal sums and nothing in the suite depends on what `tokenizers`'
Viterbi does with a tie: candidates by start ascending, then length ascending; a node replaced
only by a strictly better candidate, the start's unk last; f64 sums taken as
`score + best_till_here`.  Real sentencepiece models do tie (rare pieces share a floor score).
These variants make ties the rule.  Only the scores of the ordinary pieces (ids 3..31999)
change; ids 0..2 and 32000.. keep theirs, and pieces, charsmap, pre-tokenizer and template are
the base's.

  flat   every score -8.0: the sum counts pieces, every equal-count split ties
  g2     round(s / 2.0) * 2.0, a result >= 0 becomes -2.0: ties among splits of unequal counts
  g05    the same on a grid of 0.5
  u2     g2, then per piece a seeded choice of -1, 0 or +1 added to the f64's bit pattern: sums
         that tie on the grid now differ by a few f64 ulps, which an f32 score cannot carry
         (the kernels restore the ulp from a mark in the piece's slot, uni_score64) and which
         depend on the order of the additions
  u05    g05 with the same nudge

A nudged value is kept only if the host loader will take it: read back the way `tokenizers`
reads tokenizer.json (oracle_lib.json_number(repr(x)), serde_json's two-rounding parse) it has
to be negative and within one f64 ulp of its nearest f32; otherwise the grid value stays.
dropped(kind, base) reports how many nudges were taken back (none on the proxy).

The unk score is min_score - 10.  On g2 the minimum is a grid value, so the unk lies on the
grid too and a path through an unk can tie with a path through pieces; on u2 it is that grid
value or one f64 ulp beside it, like every other score.  Words with characters that have no
piece (tests: "unk ties") lean on this.

`base` is the proxy or one of the long-piece variants of make_t5_long_piece_vocab.py (v19, v32,
v64), whose new pieces take grid scores like any other piece.

Usage: python tests/golden/make_t5_tied_vocab.py KIND [BASE] [OUT_DIR]
"""
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_t5_long_piece_vocab as lp  # noqa: E402

KINDS = ("flat", "g2", "g05", "u2", "u05")
BASES = ("proxy", "v19", "v32", "v64")
STEP = {"g2": 2.0, "u2": 2.0, "g05": 0.5, "u05": 0.5}
SEED = 20250
FIRST, END = 3, 32000  # the ordinary pieces
_DROPPED = {}


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _from_bits(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def loader_accepts(x):
    """The host loader's rule (assets.cpp) on the f64 that serde_json reads from repr(x):
    negative and within one f64 ulp of its nearest f32."""
    import oracle_lib
    y = oracle_lib.json_number(repr(x))
    return y < 0.0 and abs(_bits(y) - _bits(_f32(y))) <= 1


def grid(s, step):
    g = round(s / step) * step
    return -step if g >= 0 else g


def build(kind, base="proxy"):
    """The tokenizer dict of `base` with the scores of ids 3..31999 rewritten as `kind` says."""
    if kind not in KINDS or base not in BASES:
        raise ValueError((kind, base))
    if base == "proxy":
        with open(lp.TEMPLATE, encoding="utf-8") as f:
            tok = json.load(f)
    else:
        tok = lp.build(base)
    vocab = tok["model"]["vocab"]
    rng = random.Random(SEED)
    dropped = 0
    for i in range(FIRST, END):
        if kind == "flat":
            vocab[i][1] = -8.0
            continue
        g = grid(vocab[i][1], STEP[kind])
        if kind in ("u2", "u05"):
            d = rng.choice((-1, 0, 1))
            x = _from_bits(_bits(g) + d)
            if d and not loader_accepts(x):
                dropped += 1
                x = g
            g = x
        vocab[i][1] = g
    _DROPPED[(kind, base)] = dropped
    return tok


def dropped(kind, base="proxy"):
    """How many nudges build(kind, base) took back because the loader would refuse them."""
    if (kind, base) not in _DROPPED:
        build(kind, base)
    return _DROPPED[(kind, base)]


def main():
    kind = sys.argv[1]
    base = sys.argv[2] if len(sys.argv) > 2 else "proxy"
    out_dir = sys.argv[3] if len(sys.argv) > 3 else os.path.join(HERE, f"t5_{base}_{kind}")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(build(kind, base), f, ensure_ascii=False)
    print(path, "nudges dropped:", dropped(kind, base))


if __name__ == "__main__":
    main()
