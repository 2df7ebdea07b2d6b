#!/usr/bin/env python3
"""Synthetic byte-level BPE tokenizer.json files with deep, aperiodic merge tables (test
infrastructure: the fixtures of tests/test_bpe_merge_vocab.py and tests/test_gpu_bpe_paths.py).

On the gpt2 proxy vocabulary the long inputs of the GPU tests merge in one or two rounds to one
or two distinct ids, so most of what streaming_data_loader_amd/csrc/tokenize_bpe.hip does between
rounds -- compaction offsets across tiles, cached pair values next to a merge, the hand-over of
a merge across a tile edge, per-word minima in a shared wave -- cannot change their output.  The
tables built here make random words merge over a dozen and more rounds into many distinct ids.

Layout (what assets.cpp's load_byte_bpe accepts): the 256 byte symbols as ids 0..255 (id = byte
value), one id per merge after them in rank order, `<|endoftext|>` last as the one added token;
merges as [left, right] pairs, rank = position; normalizer null; ByteLevel(add_prefix_space=false,
use_regex=true) pre-tokenizer; ByteLevel post-processor.  The class table stays the project's
gpt2_classes.bin.

The merge table runs over the base alphabet a b c é 中 and a leading space (the byte symbols of
61 62 63, C3 A9, E4 B8 AD and 20), seeded:
  * é and 中 are assembled from their bytes by early merges (not rank 0), so merges start from
    byte_id of bytes >= 0x80 too, and (Ġ, x) merges from the space-prefixed first symbol;
  * every other merge joins two tokens made so far, drawn at random (short ones preferred early,
    the longest ones late, so strings of up to MAX_PIECE bytes arise), which makes the table
    rank-monotone by construction; check_monotone() asserts the loader's own condition;
  * no pair and no merged string occurs twice;
  * a self-pair of a base letter (x, x) and one of a merged token (xy, xy) sit at ranks SELF1 and
    SELF2, neither the lowest: runs like "aaa" and "aaaaa" take the left-to-right alternation in
    the middle of other merges.
Conditions on a table, asserted from the model side only (tests/bpe_merge_model.py), the seed
re-drawn (seed + 1000) until they hold: random words of 500, 1024, 1025 and 3000 symbols each take
>= MIN_ROUNDS merge rounds and give >= MIN_DISTINCT distinct ids, and at least MIN_LONG_SELF
tokens of 17..40 bytes encode to themselves (the word table's tail compare needs them), one of
them past 32 bytes.

Nothing generated is committed.  Usage: python tests/golden/make_bpe_merge_vocab.py SEED [OUT_DIR]
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import bpe_merge_model as model  # noqa: E402

SEEDS = (1011, 3023)  # both meet conditions() on their first draw
N_MERGES = 220
MAX_PIECE = 40
SELF1, SELF2 = 6, 24  # ranks of the (x, x) and (xy, xy) self-pairs
MIN_ROUNDS = 10
MIN_DISTINCT = 10
MIN_LONG_SELF = 6
COND_LENGTHS = (500, 1024, 1025, 3000)
LETTERS = [b"a", b"b", b"c", "é".encode(), "中".encode()]
SPACE = b" "
EOS = "<|endoftext|>"


def byte_symbols():
    """GPT-2 bytes_to_unicode(): the printable stand-in char of every byte."""
    out, n = [], 0
    for b in range(256):
        if 0x21 <= b <= 0x7E or 0xA1 <= b <= 0xAC or b >= 0xAE:
            out.append(chr(b))
        else:
            out.append(chr(256 + n))
            n += 1
    return out


SYM = byte_symbols()


def sym_str(raw):
    return "".join(SYM[b] for b in raw)


def random_word(rng, n, letters=LETTERS):
    """A word of exactly n bytes of whole letters, aperiodic (uniform draws)."""
    out = b""
    while len(out) < n:
        l = rng.choice(letters)
        if len(out) + len(l) <= n:
            out += l
    return out


class Table:
    """A drawn merge table: `merges` [(left bytes, right bytes)], `ids` {token bytes: id},
    `pair` {(left id, right id): (rank, merged id)}, `eos`."""

    def __init__(self, merges, seed):
        self.seed = seed
        self.merges = merges
        self.ids = {bytes([b]): b for b in range(256)}
        for l, r in merges:
            assert l + r not in self.ids, "duplicate merged string"
            self.ids[l + r] = len(self.ids)
        self.eos = len(self.ids)
        self.pair = {}
        for k, (l, r) in enumerate(merges):
            key = (self.ids[l], self.ids[r])
            assert key not in self.pair, "duplicate pair"
            self.pair[key] = (k, self.ids[l + r])
        self.strings = {i: s for s, i in self.ids.items()}

    def check_monotone(self):
        """load_byte_bpe's condition: no part of merge r is created by a merge of rank >= r."""
        creator = {l + r: k for k, (l, r) in enumerate(self.merges)}
        for k, (l, r) in enumerate(self.merges):
            assert creator.get(l, -1) < k and creator.get(r, -1) < k, f"merge {k} is not rank-monotone"

    def encode_word(self, raw):
        return model.heap_encode(list(raw), self.pair)

    def rounds(self, raw):
        ids, n = model.batch_rounds(list(raw), self.pair)
        return n, len(set(ids))

    def is_self(self, raw):
        """The vocabulary string encodes to itself: a word-table entry (assets.cpp)."""
        return raw in self.ids and self.encode_word(raw) == [self.ids[raw]]

    def self_encoding(self, lo=17, hi=MAX_PIECE):
        return [s for s in self.ids if lo <= len(s) <= hi and self.is_self(s)]

    def tokenizer(self):
        vocab = {sym_str(s): i for s, i in self.ids.items()}
        bl = {"type": "ByteLevel", "add_prefix_space": False, "trim_offsets": True, "use_regex": True}
        return {
            "version": "1.0", "truncation": None, "padding": None,
            "added_tokens": [{"id": self.eos, "content": EOS, "single_word": False, "lstrip": False,
                              "rstrip": False, "normalized": False, "special": True}],
            "normalizer": None, "pre_tokenizer": dict(bl), "post_processor": dict(bl), "decoder": dict(bl),
            "model": {"type": "BPE", "dropout": None, "unk_token": None, "continuing_subword_prefix": None,
                      "end_of_word_suffix": None, "fuse_unk": False, "byte_fallback": False,
                      "ignore_merges": False, "vocab": vocab,
                      "merges": [[sym_str(l), sym_str(r)] for l, r in self.merges]},
        }


def draw(seed):
    """One table from one seed (conditions not yet checked)."""
    rng = random.Random(seed)
    plain = list(LETTERS[:3])      # tokens a right part may be (no leading space)
    spaced = []                    # tokens with a leading space: left parts only
    have = set(plain) | {SPACE}
    pairs = set()
    merges = []

    def add(l, r, pool=True):
        if (l, r) in pairs or l + r in have or len(l + r) > MAX_PIECE:
            return False
        pairs.add((l, r))
        have.add(l + r)
        merges.append((l, r))
        if pool:  # (the first two bytes of 中 are no letter: never drawn as a part)
            (spaced if l.startswith(SPACE) else plain).append(l + r)
        return True

    e, z = LETTERS[3], LETTERS[4]
    forced = {1: (e[:1], e[1:]), 2: (z[:1], z[1:2]), 3: (z[:2], z[2:])}
    while len(merges) < N_MERGES:
        k = len(merges)
        if k in forced:
            assert add(*forced[k], pool=k != 2)
            continue
        if k == SELF1:
            x = rng.choice(LETTERS[:3])
            assert add(x, x)
            continue
        if k == SELF2:
            two = [t for t in plain if t != x + x and t.decode().isascii() and len(t) == 2]
            xy = rng.choice(two)
            assert add(xy, xy)
            continue
        late = k >= N_MERGES * 0.55
        r = rng.random()
        if r < 0.10:
            l = rng.choice(spaced) if spaced and rng.random() < 0.6 else SPACE
        elif late and r < 0.55:
            l = rng.choice(sorted(plain, key=len)[-12:])  # grow the longest strings
        elif r < 0.75:
            l = rng.choice([t for t in plain if len(t.decode()) <= 3])
        else:
            l = rng.choice(plain)
        short = [t for t in plain if len(t.decode()) <= 3]
        rt = rng.choice(short if rng.random() < 0.7 else plain)
        add(l, rt)
    return Table(merges, seed)


def conditions(t):
    """None when the table meets the module's conditions, else what it misses."""
    t.check_monotone()
    ranks = {l + r: k for k, (l, r) in enumerate(t.merges)}
    base = [(l, r) for l, r in t.merges if l == r and len(l) == 1]
    merged = [(l, r) for l, r in t.merges if l == r and len(l) > 1]
    if not base or not merged or min(ranks[l + r] for l, r in base + merged) == 0:
        return "self-pairs"
    rng = random.Random(t.seed * 7919 + 1)
    for n in COND_LENGTHS:
        for _ in range(3):
            rounds, distinct = t.rounds(random_word(rng, n))
            if rounds < MIN_ROUNDS or distinct < MIN_DISTINCT:
                return f"{n} symbols: {rounds} rounds, {distinct} distinct ids"
    long_self = t.self_encoding()
    if len(long_self) < MIN_LONG_SELF or max(map(len, long_self)) <= 32:
        return f"{len(long_self)} self-encoding tokens of 17..{MAX_PIECE} bytes"
    return None


_TABLES = {}


def table(seed):
    """The table of a seed: the first of seed, seed + 1000, ... that meets conditions()."""
    if seed not in _TABLES:
        s = seed
        for _ in range(50):
            t = draw(s)
            if conditions(t) is None:
                break
            s += 1000
        else:
            raise AssertionError(f"seed {seed}: no table met the conditions")
        _TABLES[seed] = t
    return _TABLES[seed]


def non_monotone(seed):
    """The seed's tokenizer with one merge moved ahead of the merge that creates its left part:
    the loader must refuse it."""
    t = table(seed)
    creator = {l + r: k for k, (l, r) in enumerate(t.merges)}
    k = next(k for k, (l, r) in enumerate(t.merges) if l in creator and k > creator[l] + 1)
    tok = t.tokenizer()
    m = tok["model"]["merges"]
    m.insert(creator[t.merges[k][0]], m.pop(k))
    return tok


def write(seed, out_dir, tok=None):
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(tok or table(seed).tokenizer(), f, ensure_ascii=False)
    return path


def main():
    seed = int(sys.argv[1])
    print(write(seed, sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, f"bpe_merge_{seed}")))


if __name__ == "__main__":
    main()
