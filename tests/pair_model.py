"""Sentence pairs (sdl_config.pair = 1, DESIGN.md §3 "Sentence pairs") in plain Python: the row a
pair handle gives for the tokenizer ids a, b of an example's two texts.  test_pair_model.py pins
this to tokenizers' encode(a, b) under longest_first truncation and padding to S."""
import numpy as np


def kept_lengths(n_a, n_b, S):
    """(k_a, k_b): tokenizers' TruncationStrategy::LongestFirst (right, stride 0) of n_a + n_b ids
    into M = S - 3.  On a tie A counts as the shorter side, so B gets the odd id."""
    M = S - 3
    if n_a + n_b <= M:
        return n_a, n_b
    lo, hi = min(n_a, n_b), max(n_a, n_b)
    hi = lo if lo > M else max(lo, M - lo)
    if lo + hi > M:
        lo, hi = M // 2, M // 2 + M % 2
    return (lo, hi) if n_a <= n_b else (hi, lo)


def pair_row(a, b, S, cls, sep):
    """(input_ids, token_type_ids, attention_mask) of one pair, int32 [S] each."""
    k_a, k_b = kept_lengths(len(a), len(b), S)
    ids = [cls] + list(a[:k_a]) + [sep] + list(b[:k_b]) + [sep]
    tt = [0] * (k_a + 2) + [1] * (k_b + 1)
    n = len(ids)
    out = np.zeros((3, S), np.int32)
    out[0, :n] = ids
    out[1, :n] = tt
    out[2, :n] = 1
    return out[0], out[1], out[2]


def pair_rows(pairs_of_ids, S, cls, sep):
    """The planes of many pairs: (input_ids, token_type_ids, attention_mask), int32 [n, S]."""
    n = len(pairs_of_ids)
    ids, tt, am = (np.zeros((n, S), np.int32) for _ in range(3))
    for r, (a, b) in enumerate(pairs_of_ids):
        ids[r], tt[r], am[r] = pair_row(a, b, S, cls, sep)
    return ids, tt, am
