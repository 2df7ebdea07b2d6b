"""A model of the packed span rows (sdl_config.pack = 1 under the span task, include/sdl_batcher.h
"Packed span rows"): pack_model's stream (eos = </s>, chunk length N, ids only) cut into chunks, then
span_noise_model's policy row on every chunk as chunk 0 of record q, the row's packed index.  A
helper module, not a test.

span_noise_model.row takes a row of at most W ids and gives W / 4 labels; a chunk has N > S ids, so
it is called at the width W = N rounded up to 4 and the planes are cut to S and S / 4 -- everything
behind the cut must be the fill values, which is the contract's "the corrupted chunk fits the row".
It asserts the round trip (unspan) on every row it makes."""
import numpy as np

import pack_model
import span_noise_model as M

MAX_N = 3584  # the chunk length k_pack_span_rows' LDS layout holds
EMPTY = np.zeros(0, np.int32)


def chunk_length(S, per_mille, mean):
    """N: the last n in 1..65535 before the first n with u(n) + m(n) > S; None where create refuses
    the config (labels, sentinels, the kernel's layout)."""
    N = 0
    for n in range(1, 65536):
        t, m = M.counts(n, per_mille, mean)
        if n - t + m > S:
            break
        N = n
    t, m = M.counts(N, per_mille, mean)
    return None if t + m + 1 > S // 4 or m + 1 > 100 or N > MAX_N else N


def row(chunk, S, seed, q, per_mille, mean):
    """One chunk's planes: input_ids [S], attention_mask [S], labels [S // 4]."""
    W = max(len(chunk) + (-len(chunk)) % 4, S + (-S) % 4)
    ids, am, lab, _ = M.row(list(chunk), W, seed, q, 0, per_mille, mean)
    assert (ids[S:] == 0).all() and (am[S:] == 0).all() and (lab[S // 4:] == -100).all(), (len(chunk), S)
    return ids[:S], am[:S], lab[:S // 4]


def _stack(rows, S):
    if not rows:
        return tuple(np.zeros((0, w), np.int32) for w in (S, S, S // 4))
    return tuple(np.stack(p) for p in zip(*rows))


def pack(id_lists, S, per_mille, mean, seed, min_ids=0, carry=EMPTY, q0=0):
    """One call: -> ((input_ids [G, S], attention_mask [G, S], labels [G, S // 4]), new carry).
    q0: packed rows the handle emitted before the call."""
    N = chunk_length(S, per_mille, mean)
    chunks, _, _, _, new = pack_model.pack(id_lists, N, M.tok().eos, min_ids, (carry, np.zeros(len(carry), np.int32)))
    return _stack([row(c, S, seed, q0 + g, per_mille, mean) for g, c in enumerate(chunks)], S), new[0]


def flush(carry, S, per_mille, mean, seed, q):
    """The flush row: planes of 0 or 1 rows, the carry's c ids corrupted with n = c and packed index q."""
    return _stack([row(carry, S, seed, q, per_mille, mean)] if len(carry) else [], S)


record_rows = pack_model.record_rows
