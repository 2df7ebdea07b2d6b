"""A plain model of the best-fit rows (sdl_batcher_set_best_fit, include/sdl_batcher.h "Best-fit
rows"): a sorted tail list, a dict of stacks by room and a linear search for the least room >= l."""
import numpy as np

import pack_model


def pack(id_lists, S, eos, W, min_ids=0):
    """One call: -> (input_ids, attention_mask, labels, position_ids, placements); planes [G, S].
    A placement is (exact, tie, moved, new): the tail filled its row exactly; at least two open rows
    shared the chosen room; ... and the most recent of them is not the one of lowest index; the tail
    opened a row."""
    rows, placements = [], []  # a row: its pieces, in placement order
    for k in range(0, len(id_lists), W):
        tails = []
        for i, t in enumerate(id_lists[k:k + W]):
            if not pack_model.kept(len(t), min_ids):
                continue
            seg = list(t) + [eos]
            full = len(seg) // S
            rows += [[seg[c * S:(c + 1) * S]] for c in range(full)]
            if len(seg) % S:
                tails.append((i, seg[full * S:]))
        tails.sort(key=lambda it: (-len(it[1]), it[0]))
        stacks = {}  # room -> the open rows that have it, the most recent last
        for _, t in tails:
            room = next((c for c in range(len(t), S) if stacks.get(c)), None)
            if room is None:
                rows.append([])
                g, room = len(rows) - 1, S
                placements.append((False, False, False, True))
            else:
                g = stacks[room][-1]
                placements.append((room == len(t), len(stacks[room]) > 1, g != min(stacks[room]), False))
                stacks[room].pop()
            rows[g].append(t)
            if room > len(t):
                stacks.setdefault(room - len(t), []).append(g)
    # a row is its pieces and, behind them, the flush row's values
    planes = [pack_model.flush(pack_model.EMPTY, S)]  # (no rows: planes [0, S])
    for pieces in rows:
        ids = np.array([x for p in pieces for x in p], np.int32)
        pos = np.array([x for p in pieces for x in range(len(p))], np.int32)
        planes.append(pack_model.flush((ids, pos), S))
    return (*[np.concatenate(p) for p in zip(*planes)], placements)
