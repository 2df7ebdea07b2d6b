#!/usr/bin/env python3
"""t5 Unigram tokenizer.json variants with pieces longer than 16 bytes (test infrastructure:
the fixtures of tests/test_t5_long_pieces.py and tests/test_gpu_unigram_paths.py).

The t5 proxy asset has no piece past 16 bytes (longest plain piece 16, longest "▁" payload
15), so three parts of streaming_data_loader_amd/csrc/tokenize_unigram.hip never run on it:
the wide Viterbi's rows of pieces past 16 bytes (two-block hash, pool tail compare), the
`wide_ok == false` route that makes every 17..48-byte word a long item, and the
k_unigram_long<32> / <64> instantiations.  A SentencePiece model trained with a larger
max_sentencepiece_length reaches them; these variants do so in tests.

Each variant is the proxy asset with its lowest-scored ordinary pieces (ids 3..31999: not
<pad> </s> <unk>, not <extra_id_k>) replaced by new pieces.  A new piece is a concatenation
of existing printable-ASCII proxy pieces (seeded RNG) cut to the wanted length, so every
substring of it competes with real pieces, and carries a score around -8 (the f32 grid, as
the proxy's own scores), so it wins the Viterbi where it occurs.  Nothing else changes:
sizes, special ids, the Precompiled charsmap, WhitespaceSplit + Metaspace, the template.

  v19       48 plain pieces of 17, 18 and 19 bytes and six "▁" pieces with payloads of
            14..16 bytes: maxlen_first 19, maxlen_meta 16 -- the wide Viterbi stays on.
            Five pairs share their length and first 16 bytes (the same slot header; their
            hashes differ, so a probe for one does not meet the other -- collisions() below
            finds the strings that do meet a piece's slot); six start with the first 4 bytes of a frequent short piece (the prefix
            bound of that 4-byte key has to rise to their length).
  v32       plain pieces of 20..32 bytes, "▁" payloads of 17..31: the wide Viterbi is off.
  v64       plain pieces of 33..64 bytes, "▁" payloads of 32..63.
  too_long  one plain piece of 65 bytes: the loader must refuse it.

Usage: python tests/golden/make_t5_long_piece_vocab.py VARIANT [OUT_DIR]
"""
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
TEMPLATE = os.path.join(REPO, "streaming_data_loader_amd", "assets", "t5_proxy", "tokenizer.json")
META = "▁"
VARIANTS = ("v19", "v32", "v64")
SEEDS = {"v19": 1901, "v32": 3201, "v64": 6401, "too_long": 6501}
N_PAIRS = 5   # v19: pairs sharing their first 16 bytes
N_PFX = 6     # v19: pieces starting with a frequent short piece's first 4 bytes


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def _lengths(variant):
    """(plain piece lengths, "▁" payload lengths) of a variant."""
    if variant == "v19":
        return [17, 18, 19] * 16, [14, 15, 16] * 2
    if variant == "v32":
        return list(range(20, 33)) * 3, list(range(17, 32))
    if variant == "v64":
        return list(range(33, 65)), list(range(32, 64))
    if variant == "too_long":
        return [65], []
    raise ValueError(variant)


def plan(variant, template=TEMPLATE):
    """The variant's new pieces: {"plain": [...], "meta": [payloads...], "pairs": [(a, b)...],
    "pfx": [...]} (pairs and pfx are members of plain), all printable ASCII."""
    with open(template, encoding="utf-8") as f:
        vocab = json.load(f)["model"]["vocab"]
    have = {p for p, _ in vocab}
    ascii_plain = [(p, s) for p, s in vocab[3:32000]
                   if not p.startswith(META) and all(0x21 <= ord(c) <= 0x7E for c in p)]
    parts = [p for p, _ in ascii_plain]
    rng = random.Random(SEEDS[variant])

    def cat(n, head=""):
        s = head
        while len(s) < n:
            s += rng.choice(parts)
        return s[:n]

    made = set()

    def fresh(n, head="", meta=False):
        while True:
            s = cat(n, head)
            full = META + s if meta else s
            if full not in have and full not in made:
                made.add(full)
                return s

    plain_lens, meta_lens = _lengths(variant)
    plain, pairs, pfx = [], [], []
    todo = list(plain_lens)
    if variant == "v19":
        # pairs: the same length and first 16 bytes (the same slot key), another tail
        for _ in range(N_PAIRS):
            n = todo.pop(0)
            todo.remove(n)
            a = fresh(n)
            b = fresh(n, head=a[:16])
            pairs.append((a, b))
            plain += [a, b]
        # frequent short pieces of >= 4 bytes (by score) lend their first 4 bytes
        heads = [p for p, _ in sorted(ascii_plain, key=lambda e: -e[1]) if 4 <= len(p) <= 8][:N_PFX]
        for h in heads:
            s = fresh(todo.pop(0), head=h[:4])
            pfx.append(s)
            plain.append(s)
    plain += [fresh(n) for n in todo]
    meta = [fresh(n, meta=True) for n in meta_lens]
    return {"plain": plain, "meta": meta, "pairs": pairs, "pfx": pfx}


def build(variant, template=TEMPLATE):
    """The tokenizer dict of a variant; `new_ids(variant)` gives the ids the new pieces took."""
    with open(template, encoding="utf-8") as f:
        tok = json.load(f)
    vocab = tok["model"]["vocab"]
    pl = plan(variant, template)
    new = pl["plain"] + [META + m for m in pl["meta"]]
    # the lowest-scored ordinary pieces give up their slots (stable among equal scores)
    victims = sorted(range(3, 32000), key=lambda i: vocab[i][1])[:len(new)]
    for k, (i, p) in enumerate(zip(sorted(victims), new)):
        vocab[i] = [p, _f32(-8.0 - 0.0078125 * (k % 64))]
    assert len({p for p, _ in vocab}) == len(vocab)  # no duplicate strings
    return tok


def new_ids(variant, template=TEMPLATE):
    """{piece string ("▁" included): id} of the variant's new pieces."""
    pl = plan(variant, template)
    new = set(pl["plain"]) | {META + m for m in pl["meta"]}
    return {p: i for i, (p, _) in enumerate(build(variant, template)["model"]["vocab"]) if p in new}


# ---- strings that collide with a new piece in the vocabulary's cuckoo table -------------------
# The kernels find a piece longer than 16 bytes by a hash over all its bytes (common.hpp: ph_init,
# ph_mix, ph_final; assets.cpp: piece_hash), read the two slots the hash names (cuckoo_slot1 /
# cuckoo_slot2) and accept a slot whose header -- length, kind, first 16 bytes -- matches once
# the bytes past 16 equal the pool's.  A string that shares a piece's length and first 16 bytes
# names two *other* slots, so the compare of the tail only ever rejects anything for a string
# whose hash also names the slot the piece sits in.  collisions() searches such strings: the
# piece with its last three bytes replaced, one of its slot indices equal to one of the piece's
# on COLLIDE_BITS bits (the table has 2^16 .. 2^18 slots for a 32,100-piece vocabulary; equal
# low 18 bits are equal under every such mask).  Which of its two slots the table builder gave
# the piece is not restated here: the strings come in both kinds, so one of each pair meets it.
M32 = 0xFFFFFFFF
COLLIDE_BITS = 18
UC_PIECE = 0


def ph_init(n, cont):
    return (((n * 2 + cont) * 0x9E3779B1) & M32) ^ 0x7F4A7C15


def ph_mix(h, w):
    h = ((h ^ w) * 0x85EBCA6B) & M32
    return h ^ (h >> 13)


def ph_final(h):
    h ^= h >> 16
    h = (h * 0x7FEB352D) & M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & M32
    return h ^ (h >> 16)


def cuckoo_slot1(h, mask):
    return h & mask


def cuckoo_slot2(h, mask):
    g = (((h >> 16) | (h << 16)) & M32) * 0xD35A2D97 & M32
    g ^= g >> 15
    return g & mask


def piece_hash(payload, cont=UC_PIECE):
    """assets.cpp piece_hash: zero-padded 16-byte blocks, 4 little-endian dwords each."""
    h = ph_init(len(payload), cont)
    for b0 in range(0, max(len(payload), 1), 16):
        blk = payload[b0:b0 + 16].ljust(16, b"\0")
        for i in range(4):
            h = ph_mix(h, int.from_bytes(blk[4 * i:4 * i + 4], "little"))
    return ph_final(h)


def piece_slots(payload, bits=COLLIDE_BITS):
    h = piece_hash(payload)
    return cuckoo_slot1(h, (1 << bits) - 1), cuckoo_slot2(h, (1 << bits) - 1)


_COLLISIONS = {}


def collisions(variant, template=TEMPLATE):
    """[(piece, string, k, j)]: `string` has the piece's length and all but its last three bytes,
    is no piece itself, and its slot k (1 or 2) equals the piece's slot j on COLLIDE_BITS bits.
    For every plain piece of 19..32 bytes (the changed bytes lie in its second 16-byte block)
    and every (k, j), the first such string in a fixed enumeration, where one exists."""
    if variant in _COLLISIONS:
        return _COLLISIONS[variant]
    import numpy as np
    pl = plan(variant, template)
    have = set(pl["plain"])
    mask = (1 << COLLIDE_BITS) - 1
    alpha = np.array([c for c in range(0x21, 0x7F) if c not in (0x3C, 0x3E)], np.uint64)  # no "<" ">"
    t0, t1, t2 = (x.ravel() for x in np.meshgrid(alpha, alpha, alpha, indexing="ij"))
    m32 = np.uint64(M32)

    def mix(h, w):
        h = ((h ^ w) * np.uint64(0x85EBCA6B)) & m32
        return h ^ (h >> np.uint64(13))

    out = []
    for p in pl["plain"]:
        n = len(p)
        if not 19 <= n <= 32:
            continue
        raw = p.encode()
        h = ph_init(n, UC_PIECE)
        for i in range(4):
            h = ph_mix(h, int.from_bytes(raw[4 * i:4 * i + 4], "little"))
        # the second block of every candidate: the piece's bytes with the last three replaced
        blk = np.zeros((len(t0), 16), np.uint8)
        blk[:, :n - 16] = np.frombuffer(raw[16:], np.uint8)
        blk[:, n - 19], blk[:, n - 18], blk[:, n - 17] = t0, t1, t2
        words = blk.view("<u4").astype(np.uint64)
        hv = np.full(len(t0), h, np.uint64)
        for i in range(4):
            hv = mix(hv, words[:, i])
        hv ^= hv >> np.uint64(16)
        hv = (hv * np.uint64(0x7FEB352D)) & m32
        hv ^= hv >> np.uint64(15)
        hv = (hv * np.uint64(0x846CA68B)) & m32
        hv ^= hv >> np.uint64(16)
        s1 = hv & np.uint64(mask)
        g = (((hv >> np.uint64(16)) | (hv << np.uint64(16))) & m32) * np.uint64(0xD35A2D97) & m32
        g ^= g >> np.uint64(15)
        s2 = g & np.uint64(mask)
        mine = piece_slots(raw)
        for k, sv in ((1, s1), (2, s2)):
            for j in (1, 2):
                for x in np.flatnonzero(sv == np.uint64(mine[j - 1])):
                    s = p[:-3] + chr(int(t0[x])) + chr(int(t1[x])) + chr(int(t2[x]))
                    if s != p and s not in have:
                        out.append((p, s, k, j))
                        break
    _COLLISIONS[variant] = out
    return out


def main():
    variant = sys.argv[1]
    out_dir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "t5_" + variant)
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(build(variant), f, ensure_ascii=False)
    print(path)


if __name__ == "__main__":
    main()
