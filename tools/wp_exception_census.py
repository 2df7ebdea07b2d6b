#!/usr/bin/env python3
"""Share of WordPiece chunks without an exception (every piece exactly one id), the chunks whose
id list tokenize_wordpiece.hip step 5 gathers through the piece descriptors, counted on the CPU.

    python tools/wp_exception_census.py [--mib 16] [fixture] [heldout]

The corpus' records are tiled the way bench.py tiles them (seeded permutations) up to --mib of
text; a word is given to the 1,024-byte chunk of its first byte.  Words are split the way
BertPreTokenizer splits the normalized text, closely enough for a census: runs of word chars,
every other non-space char (and every CJK ideograph) alone; a word's ids are the CPU oracle's."""
import argparse
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

CHUNK = 1024
CJK = "㐀-䶿一-鿿豈-﫿\U00020000-\U0002fa1f"
WORD_RE = re.compile(f"[{CJK}]|[^\\W_{CJK}]+|[^\\w\\s]|_")


def census(corpus, mib):
    import bench
    import oracle_lib
    tok = oracle_lib.Tok()
    records = bench.corpus_records(corpus)
    order = bench.build_order(records, mib << 20, seed=0)
    per_record = []  # (byte offset in the record, ids) of every word
    for text in records:
        words, at, done = [], 0, 0
        for m in WORD_RE.finditer(text):
            at += len(text[done:m.start()].encode("utf-8"))
            done = m.start()
            words.append((at, m.group()))
        per_record.append((len(text.encode("utf-8")), words))
    cache = {}
    chunks = {}  # chunk -> [pieces, exceptions]
    base = 0
    for i in order:
        n, words = per_record[i]
        for at, w in words:
            k = cache.get(w)
            if k is None:
                k = cache[w] = len(tok.encode(w)) - 2
            c = chunks.setdefault((base + at) // CHUNK, [0, 0])
            c[0] += 1
            c[1] += k != 1
        base += n
    n_chunks = (base + CHUNK - 1) // CHUNK
    plain = n_chunks - sum(1 for c in chunks.values() if c[1])
    pieces = sum(c[0] for c in chunks.values())
    exc = sum(c[1] for c in chunks.values())
    print(f"{corpus}: {n_chunks} chunks of {base} bytes, {pieces / n_chunks:.1f} words a chunk, "
          f"{exc / n_chunks:.2f} words of != 1 id a chunk, {plain} chunks without one ({100.0 * plain / n_chunks:.2f} %)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=16)
    ap.add_argument("corpora", nargs="*", default=["fixture", "heldout"])
    a = ap.parse_args()
    for c in a.corpora:
        census(c, a.mib)
