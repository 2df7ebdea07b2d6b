"""The BERT masking policies (sdl_config.mask_policy 1 / 2), applied literally as DESIGN.md §3
"Masking policies" states them: the model the device rows are compared with.  A helper module,
not a test.

Unmasked rows come from the CPU oracle run with mask_length = 0; this module picks and replaces.
The Philox is the contract's (tests/golden/make_goldens.py philox4x32_10, oracle/sdl_oracle.c),
restated over numpy arrays and pinned to the oracle's orc_mlm_key by test_mlm_policy_model.py."""
import functools
import random

import numpy as np

import oracle_lib

M32 = 0xFFFFFFFF
DRAW_DOMAIN, RANDOM_DOMAIN = 0x20000000, 0x30000000  # or-ed into the chunk word of the counter
MASK_BELOW, RANDOM_BELOW = 0xCCCCCCCD, 0xE6666667  # u < ...: [MASK] (80 %), else a random id (10 %)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays of counters (uint64 arithmetic on 32-bit words)."""
    c0, c1, c2, c3 = (np.asarray(x, np.uint64) & M32 for x in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0 & M32), np.uint64(k1 & M32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ k0) & M32, p1 & M32, ((p0 >> np.uint64(32)) ^ c3 ^ k1) & M32, p0 & M32
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def row_words(seed, rec, chunk_word, S):
    """Word pos & 3 of counter (pos >> 2, chunk_word, rec lo, rec hi) for pos in 0..S."""
    q = np.arange((S + 3) // 4, dtype=np.uint64)
    z = np.zeros_like(q)
    w = philox4x32_10(q, z + np.uint64(chunk_word), z + np.uint64(rec & M32), z + np.uint64(rec >> 32), seed & M32,
                      seed >> 32)
    return np.stack(w, axis=1).reshape(-1)[:S]


@functools.lru_cache(maxsize=None)
def proxy_vocab():
    """(vocab_size, continuation flags, cls, sep) of the bert proxy vocabulary."""
    with open(oracle_lib.VOCAB_TXT, encoding="utf-8") as f:
        pieces = f.read().split("\n")
    if pieces and pieces[-1] == "":
        pieces.pop()
    cont = np.array([p.startswith("##") for p in pieces], bool)
    cont.setflags(write=False)
    return len(pieces), cont, pieces.index("[CLS]"), pieces.index("[SEP]")


def budget(l, ncand, mask_length, per_mille):
    return 0 if ncand == 0 else min(mask_length, max(1, (l * per_mille + 500) // 1000))


def pick(ids, l, keys, policy, mask_length, per_mille, excluded, cont):
    """The contract's candidates, units, budget, order and pick for one row.  Returns
    (selected positions, info) with info = dict(k, units, skipped, taken)."""
    cand = [j < l and int(ids[j]) not in excluded for j in range(len(ids))]
    units = []  # lists of positions
    for j in range(l):
        if not cand[j]:
            continue
        if policy == 2 and cont[int(ids[j])] and j > 0 and cand[j - 1]:
            units[-1].append(j)
        else:
            units.append([j])
    k = budget(l, sum(cand), mask_length, per_mille)
    taken, skipped, sel = 0, 0, []
    for u in sorted(units, key=lambda u: (int(keys[u[0]]), u[0])):
        if taken >= k:
            break
        if len(u) > k - taken:
            skipped += 1
            continue
        sel += u
        taken += len(u)
    return sorted(sel), {"k": k, "units": units, "skipped": skipped, "taken": taken}


def unmasked_rows(texts, S, min_ids=64, B=64):
    """The oracle's rows with mask_length = 0, as [4, G, S] (ids, attention, token types, labels),
    and each row's (record, chunk, filled positions l)."""
    tok = oracle_lib.Tok()
    ob = oracle_lib.OracleBatcherEx(oracle_lib.Encoder("bert", tok), oracle_lib.MLM, B, S, mask_length=0,
                                    min_ids=min_ids)
    out, where = [], []

    def take(d):
        if d is not None and d["rows"]:
            out.append(np.stack([d[k][:d["rows"]] for k in ("input_ids", "attention_mask", "token_type_ids", "labels")]))
    for r, t in enumerate(texts):
        take(ob.push(t))
        n = len(tok.encode(t)) + 3  # encode gives [CLS] ids [SEP]; the framing adds a [CLS] and two [SEP]
        if n >= min_ids:
            where += [(r, c, min(S, n - c * S)) for c in range(-(-n // S))]
    while True:
        d = ob.flush()
        if d is None or not d["rows"]:
            break
        take(d)
    rows = np.concatenate(out, axis=1) if out else np.zeros((4, 0, S), np.int32)
    assert rows.shape[1] == len(where), (rows.shape, len(where))
    return rows, where


def apply(rows, where, policy, seed, mask_length, per_mille=150, mask_id=103, first_record=0):
    """Policy 1 / 2 over unmasked rows: (masked [4, G, S] planes, per-row info with `sel`)."""
    vocab_size, cont, cls, sep = proxy_vocab()
    excluded = {0, mask_id, cls, sep}
    got = rows.copy()
    S = rows.shape[2]
    infos = []
    for g, (r, c, l) in enumerate(where):
        rec = first_record + r
        ids = rows[0, g]
        assert (ids[l:] == 0).all() and (ids[:l] != 0).all()
        sel, info = pick(ids, l, row_words(seed, rec, c, S), policy, mask_length, per_mille, excluded, cont)
        info["sel"] = sel
        if sel:
            u = row_words(seed, rec, c | DRAW_DOMAIN, S)
            rr = row_words(seed, rec, c | RANDOM_DOMAIN, S)
            for j in sel:
                got[3, g, j] = ids[j]
                if int(u[j]) < MASK_BELOW:
                    got[0, g, j] = mask_id
                elif int(u[j]) < RANDOM_BELOW:
                    got[0, g, j] = (int(rr[j]) * vocab_size) >> 32
        infos.append(info)
    return got, infos


# ---- the synthetic text of the issue's property and GPU cases ---------------------------------
COMMON = ("the of and to in a is that for it as was with be by on not he this are or his from at which but have an "
          "had they you were their one all we can her has there been if more when will would who so no").split()


def random_word(rng):
    return "".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(3, 18)))


def synthetic_texts(seed=5, n=40, lo=40, hi=400):
    """n records of lo..hi words, half random 3-18 letter words (many pieces each) and half
    common words, plus a record of two long piece runs (15 and 9 pieces in the proxy vocabulary)."""
    rng = random.Random(seed)
    texts = [" ".join(random_word(rng) if rng.random() < 0.5 else rng.choice(COMMON)
                      for _ in range(rng.randint(lo, hi))) for _ in range(n)]
    texts.append("zqxjkvzqxjkvzqxjkv qzvxkjwqzvxkjw")
    return texts
