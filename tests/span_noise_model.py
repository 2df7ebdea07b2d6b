"""T5's span corruption (sdl_config.span_policy 1), applied literally as DESIGN.md §3 "Span
policies" states it: the model the device rows are compared with.  A helper module, not a test.

Row ids are [eos] + T5Tok.encode(text) + [eos] (encode ends with the template's </s>), cut at S;
the Philox is mlm_policy_model's.  Every row is checked on the way: spans of at least one id and
the round trip -- each sentinel of input_ids replaced by its label segment gives back the ids."""
import functools
import json
import math
import os

import numpy as np

import oracle_lib
from mlm_policy_model import row_words

NOISE_DOMAIN, KEEP_DOMAIN = 0x50000000, 0x60000000  # or-ed into the chunk word of the counter
HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def tok():
    return oracle_lib.T5Tok()


@functools.lru_cache(maxsize=None)
def extra_ids():
    """The ids of <extra_id_0..99> (a row's closing sentinel is extra[m], m <= 99)."""
    t = tok()
    ids = [t.special_id(f"<extra_id_{k}>") for k in range(100)]
    assert all(i >= 0 for i in ids) and len(set(ids)) == 100
    return tuple(ids)


def counts(n, per_mille, mean):
    """(t noise ids, m spans) of a row of n ids."""
    if n < 2:
        return 0, 0
    t = min(max((n * per_mille + 500) // 1000, 1), n - 1)
    m = min(max(1, math.floor(t / mean + 0.5)), t, n - t)
    return t, m


def capacity(S, per_mille, mean):
    """(labels needed, sentinels needed) by a full row."""
    t, m = counts(S, per_mille, mean)
    return t + m + 1, m + 1


def composition(seed, rec, chunk, domain, total, m):
    """`total` cut into m parts of at least one: the m - 1 smallest (key, i) over i in 1..total-1."""
    if m <= 1:
        return [total] if m == 1 else []
    key = row_words(seed, rec, chunk | domain, total)  # key[i]: word i & 3 of counter i >> 2
    cuts = sorted(sorted(range(1, total), key=lambda i: (int(key[i]), i))[:m - 1])
    edges = [0] + cuts + [total]
    return [edges[s + 1] - edges[s] for s in range(m)]


def unspan(inp, lab):
    """The round trip: every sentinel of `inp` replaced by its label segment -> (ids, sentinels
    replaced).  Labels are cut at <extra_id_0>, <extra_id_1>, ... in that order; the last cut is
    the closing sentinel.  (Ids that hold literal sentinels of their own are not told apart.)"""
    extra, segs = extra_ids(), []
    for x in lab:
        if len(segs) < len(extra) and x == extra[len(segs)]:
            segs.append([])
        else:
            segs[-1].append(x)
    assert segs and not segs[-1]
    out, k = [], 0
    for x in inp:
        if k < len(segs) - 1 and x == extra[k]:
            out += segs[k]
            k += 1
        else:
            out.append(x)
    return out, k


def row(ids, S, seed, rec, chunk, per_mille, mean):
    """One row's planes (input_ids [S], attention_mask [S], labels [S // 4]) and (a, b)."""
    n, LW, extra = len(ids), S // 4, extra_ids()
    assert 1 <= n <= S
    t, m = counts(n, per_mille, mean)
    u = n - t
    b = composition(seed, rec, chunk, NOISE_DOMAIN, t, m)
    a = composition(seed, rec, chunk, KEEP_DOMAIN, u, m)
    assert len(a) == len(b) == m and all(x >= 1 for x in a + b) and sum(b) == t and sum(a) == (u if m else 0)
    assert t + m + 1 <= LW and m + 1 <= 100, (n, t, m, LW)
    inp, lab, at = [], [], 0
    for s in range(m):
        inp += list(ids[at:at + a[s]]) + [extra[s]]
        lab += [extra[s]] + list(ids[at + a[s]:at + a[s] + b[s]])
        at += a[s] + b[s]
    if m == 0:
        inp, at = [ids[0]], 1
    lab.append(extra[m])
    assert at == n and len(inp) == u + m and len(lab) == t + m + 1
    back, k = unspan(inp, lab)
    assert back == list(ids) and k == m, (rec, chunk)
    L = len(inp)
    out_i = np.zeros(S, np.int32)
    out_i[:L] = inp
    out_a = (np.arange(S) < L).astype(np.int32)
    out_l = np.full(LW, -100, np.int32)
    out_l[:len(lab)] = lab
    return out_i, out_a, out_l, (a, b)


def record_ids(text):
    t = tok()
    return [t.eos] + t.encode(text) + [t.eos]


def rows(texts, S, per_mille, mean, seed, first_record=0, min_ids=64):
    """Every row of `texts` in order: planes dict ([G, S], [G, S], [G, S // 4]) and per-row info
    dicts (rec, chunk, n, a, b)."""
    planes, info = ([], [], []), []
    for r, text in enumerate(texts):
        ids = record_ids(text)
        if len(ids) < min_ids:
            continue
        for c in range(-(-len(ids) // S)):
            part = ids[c * S:(c + 1) * S]
            i, am, lab, (a, b) = row(part, S, seed, first_record + r, c, per_mille, mean)
            for p, x in zip(planes, (i, am, lab)):
                p.append(x)
            info.append({"rec": r, "chunk": c, "n": len(part), "a": a, "b": b})
    G = len(info)
    shape = ((G, S), (G, S), (G, S // 4))
    out = {k: (np.stack(p) if G else np.zeros(sh, np.int32))
           for k, p, sh in zip(("input_ids", "attention_mask", "labels"), planes, shape)}
    return out, info


def padded(planes, B):
    """The planes with the last batch's unfilled rows at T5Data::new's values (0, 1, -100)."""
    G = planes["input_ids"].shape[0]
    pad = (-G) % B

    def ext(a, v):
        return np.concatenate([a, np.full((pad, a.shape[1]), v, np.int32)])
    return {"input_ids": ext(planes["input_ids"], 0), "attention_mask": ext(planes["attention_mask"], 1),
            "labels": ext(planes["labels"], -100)}


@functools.lru_cache(maxsize=None)
def fixture_records():
    with open(os.path.join(HERE, "golden", "test_records.jsonl"), encoding="utf-8") as f:
        return tuple(json.loads(l)["text"] for l in f)


WORDS = ("the", "of", "and", "a", "in", "to", "is", "was", "it", "for")


def grown_record(target, seed=0):
    """A record grown word by word until it has exactly `target` framed ids (>= 3)."""
    assert target >= 3
    text, k = "", seed
    while len(record_ids(text)) < target:
        for step in range(len(WORDS)):
            cand = (text + " " + WORDS[(k + step) % len(WORDS)]).strip()
            if len(record_ids(cand)) <= target:
                text = cand
                break
        else:
            raise AssertionError(f"cannot reach {target} ids from {len(record_ids(text))}")
        k += 1
    assert len(record_ids(text)) == target
    return text
