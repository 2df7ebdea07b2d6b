"""A numpy model of the packed clm rows (sdl_config.pack = 1, include/sdl_batcher.h "Packed rows").

The carry is what a call leaves for the next one on the same handle: (ids, position_ids), both
int32 arrays of fewer than S entries -- the positions, not only the ids, because a document's end
is a record's end and cannot be found again by comparing ids with eos.
"""
import numpy as np

EMPTY = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def kept(n, min_ids):
    """Record filter on the framed count: n ids and one trailing eos."""
    return n >= 1 and n + 1 >= min_ids


def pack(id_lists, S, eos, min_ids=0, carry=EMPTY):
    """One call: -> (input_ids, attention_mask, labels, position_ids, new_carry), planes [G, S]."""
    ids = [np.asarray(carry[0], np.int32)]
    starts = []  # stream position where each kept document starts
    at = len(carry[0])
    for t in id_lists:
        if not kept(len(t), min_ids):
            continue
        starts.append(at)
        ids.append(np.asarray(list(t) + [eos], np.int32))
        at += len(t) + 1
    stream = np.concatenate(ids) if ids else np.zeros(0, np.int32)
    L = len(stream)
    # position within the document, restarting at every row start
    pos = np.zeros(L, np.int32)
    c = len(carry[0])
    pos[:c] = carry[1]
    doc = np.zeros(L, np.int64)
    for s in starts:
        doc[s:] = s
    p = np.arange(L, dtype=np.int64)
    row0 = p // S * S
    pos[c:] = (p - np.maximum(doc, row0))[c:]
    G = L // S
    rows = stream[:G * S].reshape(G, S)
    new_carry = (stream[G * S:].copy(), (p - np.maximum(doc, G * S))[G * S:].astype(np.int32))
    if G == 0:  # the old carry stays in front with the positions it had
        new_carry[1][:c] = carry[1]
    return rows.copy(), np.ones((G, S), np.int32), rows.copy(), pos[:G * S].reshape(G, S), new_carry


def flush(carry, S):
    """The flush row(s): planes [0 or 1, S] in the plain orientation; the carry is empty afterwards."""
    c = len(carry[0])
    n = 1 if c else 0
    ids, am, lab, pos = (np.zeros((n, S), np.int32), np.zeros((n, S), np.int32), np.full((n, S), -100, np.int32),
                         np.zeros((n, S), np.int32))
    if c:
        ids[0, :c] = lab[0, :c] = carry[0]
        am[0, :c] = 1
        pos[0, :c] = carry[1]
    return ids, am, lab, pos


def record_rows(id_lists, min_ids=0):
    """sdl_device_rows.d_record_rows under pack: stream positions each record added."""
    return np.array([len(t) + 1 if kept(len(t), min_ids) else 0 for t in id_lists], np.uint32)


def unpad(ids, am, pos):
    """The documents of packed rows, from the planes alone: a document starts where position_ids == 0
    and attention_mask == 1 (documents cut by a row end come back as their pieces)."""
    docs = []
    for r in range(ids.shape[0]):
        n = int(am[r].sum())
        cuts = [i for i in range(n) if pos[r, i] == 0] + [n]
        docs += [ids[r, a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    return docs
