"""A numpy model of packed clm rows over prompt / completion examples (sdl_config.pair = 6,
include/sdl_batcher.h "Packed rows": "Prompt / completion examples"): tests/pack_model.py over the
documents a + b, and the labels from a stream of prompt flags packed the same way.

The carry is pack_model's (ids, position_ids) extended by the flags: (ids, position_ids, flags).
"""
import numpy as np

import pack_model

EMPTY = pack_model.EMPTY + (np.zeros(0, bool),)


def kept(a, b, min_ids):
    return len(b) >= 1 and len(a) + len(b) + 1 >= min_ids


def record_rows(pairs, min_ids=0):
    """sdl_device_rows.d_record_rows: stream positions each example added."""
    return np.array([len(a) + len(b) + 1 if kept(a, b, min_ids) else 0 for a, b in pairs], np.uint32)


def pack(pairs, S, eos, min_ids=0, carry=EMPTY):
    """One call over (a, b) id-list pairs: -> (input_ids, attention_mask, labels, position_ids, new_carry)."""
    docs = [(list(a), list(b)) for a, b in pairs if kept(a, b, min_ids)]
    ids, am, _, pos, (c_ids, c_pos) = pack_model.pack([a + b for a, b in docs], S, eos, 0, carry[:2])
    flags = np.concatenate([carry[2]] + [np.arange(len(a) + len(b) + 1) < len(a) for a, b in docs]).astype(bool)
    G = ids.shape[0]
    lab = np.where(flags[:G * S].reshape(G, S), -100, ids).astype(np.int32)
    return ids, am, lab, pos, (c_ids, c_pos, flags[G * S:])


def flush(carry, S):
    ids, am, lab, pos = pack_model.flush(carry[:2], S)
    if len(carry[0]):
        lab[0, :len(carry[0])][carry[2]] = -100
    return ids, am, lab, pos
