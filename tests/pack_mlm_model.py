"""A numpy model of the packed mlm rows (sdl_config.pack = 1 under the MLM task, include/sdl_batcher.h
"Packed mlm rows"): pack_model's stream over [CLS] ids [SEP] documents, then mlm_policy_model's
policy on every row as chunk 0 of record q, the row's packed index.  A helper module, not a test."""
import numpy as np

import mlm_policy_model as M
import pack_model


def pack(id_lists, S, min_ids, carry, q0, policy, seed, mask_length, per_mille=150):
    """One call: -> ([5, G, S] planes: ids, attention, token types, labels, positions; new carry).
    q0: packed rows the handle emitted before the call."""
    _, _, cls, sep = M.proxy_vocab()
    docs = [[cls] + list(t) for t in id_lists if len(t)]  # (pack_model keeps n + 2 >= min_ids of these)
    ids, am, _, pos, new_carry = pack_model.pack(docs, S, sep, min_ids, carry)
    G = ids.shape[0]
    rows = np.stack([ids, am, np.zeros_like(ids), np.full_like(ids, -100)])
    got, _ = M.apply(rows, [(q0 + g, 0, S) for g in range(G)], policy, seed, mask_length, per_mille)
    return np.concatenate([got, pos[None]]), new_carry


def flush(carry, S, q, policy, seed, mask_length, per_mille=150):
    """The flush row: [5, 0 or 1, S], the carry's c ids masked with l = c and packed index q."""
    ids, am, _, pos = pack_model.flush(carry, S)
    rows = np.stack([ids, am, np.zeros_like(ids), np.full_like(ids, -100)])
    got, _ = M.apply(rows, [(q, 0, len(carry[0]))] * ids.shape[0], policy, seed, mask_length, per_mille)
    return np.concatenate([got, pos[None]])


def record_rows(id_lists, min_ids=0):
    return np.array([len(t) + 2 if len(t) >= 1 and len(t) + 2 >= min_ids else 0 for t in id_lists], np.uint32)
