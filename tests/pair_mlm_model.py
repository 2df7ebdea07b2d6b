"""MLM sentence pairs (sdl_config.pair 2..4, DESIGN.md §3 "Sentence pairs") in plain Python: the
draw that chooses a row's two segments and its pair label, and the call's planes -- the model the
device rows are compared with.  A helper module, not a test.

Built from the two contracts it combines, imported and not edited: pair_model.py (the row of two id
lists) and mlm_policy_model.py (the Philox and the masking policies, applied to the pair rows as
chunk 0 of record first_record + r)."""
import numpy as np

import mlm_policy_model as P
import pair_model

PAIR_MLM, PAIR_MLM_NSP, PAIR_MLM_SOP = 2, 3, 4
DRAW_DOMAIN = 0x70000000  # the chunk word of the draw's Philox counter
HALF = 0x80000000


def draw_words(seed, rec):
    """The draw's Philox block (x, y, z, w): counter (0, DRAW_DOMAIN, rec lo, rec hi), key the seed."""
    w = P.philox4x32_10([0], [DRAW_DOMAIN], [rec & P.M32], [rec >> 32], seed & P.M32, seed >> 32)
    return tuple(int(v[0]) for v in w)


def draw(seed, rec, r, n_pairs, mode):
    """(first, second, label) of example r of a call over n_pairs examples with global index rec:
    the text ranges of the row's two segments (2 q is A_q, 2 q + 1 is B_q) and its pair label."""
    first, second, label = 2 * r, 2 * r + 1, 0
    if mode not in (PAIR_MLM_NSP, PAIR_MLM_SOP):
        return first, second, label
    x, y, _, _ = draw_words(seed, rec)
    if mode == PAIR_MLM_NSP:
        if x >= HALF and n_pairs >= 2:
            j = (y * (n_pairs - 1)) >> 32
            s = j + (1 if j >= r else 0)
            second, label = 2 * s + 1, 1
    elif x >= HALF:
        first, second, label = 2 * r + 1, 2 * r, 1
    return first, second, label


def chosen(pairs, mode, seed, first_record=0):
    """[(first segment, second segment, label)] of a call: `pairs` is a list of (A, B) of anything
    (texts or id lists)."""
    flat = [t for p in pairs for t in p]
    out = []
    for r in range(len(pairs)):
        f, s, lab = draw(seed, first_record + r, r, len(pairs), mode)
        out.append((flat[f], flat[s], lab))
    return out


def unmasked(pairs_of_ids, S, mode, seed, first_record=0, cls=101, sep=102):
    """The call's rows before masking: ([4, n, S] planes in mlm_policy_model's order -- ids,
    attention, token types, labels (-100) --, the pair labels [n], each row's filled positions)."""
    ch = chosen(pairs_of_ids, mode, seed, first_record)
    n = len(ch)
    ids, tt, am = pair_model.pair_rows([(a, b) for a, b, _ in ch], S, cls, sep)
    rows = np.stack([ids, am, tt, np.full((n, S), -100, np.int32)]) if n else np.zeros((4, 0, S), np.int32)
    fill = [sum(pair_model.kept_lengths(len(a), len(b), S)) + 3 for a, b, _ in ch]
    return rows, np.array([lab for _, _, lab in ch], np.int32), fill


def rows(pairs_of_ids, S, mode, policy, seed, first_record=0, mask_length=None, per_mille=150, mask_id=103, B=None):
    """The planes of one call: dict(planes=[4, G, S] (ids, attention, token types, labels),
    pair_labels=[G], infos=the masking model's per-row info).  With B, G is the pair count rounded
    up to a multiple of B and the rows past the pairs hold the unpaired mlm initial values (ids 0,
    attention 1, token types 0, labels -100) with pair label -100."""
    vocab_size, cont, cls, sep = P.proxy_vocab()
    mask_length = S if mask_length is None else mask_length
    plain, plab, fill = unmasked(pairs_of_ids, S, mode, seed, first_record, cls, sep)
    n = len(pairs_of_ids)
    where = [(r, 0, fill[r]) for r in range(n)]
    got, infos = P.apply(plain, where, policy, seed, mask_length, per_mille, mask_id, first_record)
    if B:
        G = -(-n // B) * B
        pad = np.zeros((4, G - n, S), np.int32)
        pad[1] = 1
        pad[3] = -100
        got = np.concatenate([got, pad], axis=1)
        plab = np.concatenate([plab, np.full(G - n, -100, np.int32)])
    return {"planes": got, "pair_labels": plab, "infos": infos}
