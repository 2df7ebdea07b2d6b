"""Two plain models of BPE by merge rank (test infrastructure).

`heap_encode` is tokenizers' order (models/bpe/word.rs, Word::merge_all): a heap of
(rank, position), one merge per pop, an entry skipped when its left symbol is gone, has no right
neighbour, or the pair standing there no longer merges to the id the entry was pushed with.
`batch_encode` is the form streaming_data_loader_amd/csrc/tokenize_bpe.hip uses: each round takes
the lowest rank among all adjacent pairs and merges every occurrence of it, left to right (of
overlapping occurrences the first, then every other one).  The two agree on a rank-monotone merge
table -- a merge's parts are only created by lower-ranked merges -- which is what the loader
checks; tests/test_bpe_merge_vocab.py compares them with each other, with oracle/orc_bpe.c and with
the `tokenizers` crate.  Neither shares code with the oracle or the kernels.

A table is `pair`: {(left id, right id): (rank, merged id)}.
"""
import heapq


def heap_encode(ids, pair):
    """ids: the word's byte-symbol ids.  Returns the merged ids."""
    n = len(ids)
    sym = list(ids)
    prv = list(range(-1, n - 1))
    nxt = list(range(1, n)) + [-1]
    live = [True] * n
    heap = []
    for i in range(n - 1):
        m = pair.get((sym[i], sym[i + 1]))
        if m:
            heap.append((m[0], i, m[1]))
    heapq.heapify(heap)
    while heap:
        _, pos, new = heapq.heappop(heap)
        if not live[pos] or nxt[pos] < 0:
            continue
        nx = nxt[pos]
        m = pair.get((sym[pos], sym[nx]))
        if not m or m[1] != new:
            continue  # stale
        sym[pos] = new
        live[nx] = False
        nxt[pos] = nxt[nx]
        if nxt[pos] >= 0:
            prv[nxt[pos]] = pos
        if prv[pos] >= 0:
            a = pair.get((sym[prv[pos]], sym[pos]))
            if a:
                heapq.heappush(heap, (a[0], prv[pos], a[1]))
        if nxt[pos] >= 0:
            b = pair.get((sym[pos], sym[nxt[pos]]))
            if b:
                heapq.heappush(heap, (b[0], pos, b[1]))
    return [s for s, l in zip(sym, live) if l]


def batch_rounds(ids, pair):
    """(merged ids, rounds): all occurrences of the lowest rank per round, left to right."""
    sym = list(ids)
    rounds = 0
    while len(sym) > 1:
        best = None
        for i in range(len(sym) - 1):
            m = pair.get((sym[i], sym[i + 1]))
            if m and (best is None or m[0] < best[0]):
                best = m
        if best is None:
            break
        rounds += 1
        out, i = [], 0
        while i < len(sym):
            if i + 1 < len(sym) and pair.get((sym[i], sym[i + 1])) == best:
                out.append(best[1])
                i += 2
            else:
                out.append(sym[i])
                i += 1
        sym = out
    return sym, rounds


def batch_encode(ids, pair):
    return batch_rounds(ids, pair)[0]


def split_words(text):
    """The pre-tokens of a text of letter-words joined by single spaces (`" "? letters+`): the
    first word, then every later word with its space.  text: bytes without a leading space."""
    words = text.split(b" ")
    assert all(words), "single spaces between non-empty words"
    return [words[0]] + [b" " + w for w in words[1:]]
