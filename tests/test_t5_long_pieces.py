"""The CPU oracle on vocabularies with pieces longer than 16 bytes, pinned to `tokenizers`.

tests/golden/make_t5_long_piece_vocab.py builds the t5 proxy tokenizer with a few dozen of its
lowest-scored pieces replaced by pieces of 17..19 (v19), 20..32 (v32) and 33..64 (v64) bytes.
tests/test_gpu_unigram_paths.py checks the HIP kernels against oracle/orc_unigram.c on them, so
this module first pins that oracle to the `tokenizers` crate's own output on the same
vocabularies: seeded texts of words built from the new pieces -- alone, behind a short
prefix, before a suffix, with the last byte changed -- must encode to the same ids, and the
new ids must actually occur (a reference that never chose a long piece would pin nothing).

Also here, without `tokenizers`: the generator's restatement of the vocabulary table's hash and
the strings it finds that name a new piece's slot (the inputs of the GPU cases on the tail
compare's reject side); the host loader's view of each variant (sdl_tokenizer_info_get)
and its refusal of a 65-byte piece."""
import json
import os
import random

import pytest

import make_t5_long_piece_vocab as lp
import oracle_lib

N_TEXTS = 300


def write_variant(tmp_path_factory, variant):
    path = os.path.join(str(tmp_path_factory.mktemp("t5_" + variant)), "tokenizer.json")
    with open(path, "w", encoding="utf-8") as f:
        json.dump(lp.build(variant), f, ensure_ascii=False)
    return path


@pytest.fixture(scope="module", params=lp.VARIANTS)
def variant(request, tmp_path_factory):
    return request.param, write_variant(tmp_path_factory, request.param)


def piece_texts(variant_name, n=N_TEXTS):
    """Seeded texts over the variant's new pieces ("▁" pieces by their payload: a word start)."""
    pl = lp.plan(variant_name)
    rng = random.Random(lp.SEEDS[variant_name] + 7)
    pieces = pl["plain"] + pl["meta"]
    short = ["a", "un", "re", "the", "x", "I", "pre", "1", "-", "co"]
    tails = ["s", "ing", ".", ",", "ed", "!", "42", "'s", "ly", "é"]

    def word():
        p = rng.choice(pieces)
        k = rng.randrange(5)
        if k == 0:
            return p
        if k == 1:
            return rng.choice(short) + p
        if k == 2:
            return p + rng.choice(tails)
        if k == 3:  # a near miss: the last byte changed
            return p[:-1] + ("#" if p[-1] != "#" else "%")
        return rng.choice(short) + p + rng.choice(tails)

    return [" ".join(word() for _ in range(rng.randint(3, 30))) for _ in range(n)]


def test_variant_layout():
    for name, first, meta in (("v19", (17, 19), (14, 16)), ("v32", (20, 32), (17, 31)), ("v64", (33, 64), (32, 63))):
        pl = lp.plan(name)
        v = lp.build(name)["model"]["vocab"]
        assert len(v) == 32100 and len({p for p, _ in v}) == 32100
        assert [v[i][0] for i in (0, 1, 2)] == ["<pad>", "</s>", "<unk>"]
        assert v[32099][0] == "<extra_id_0>" and v[32000][0] == "<extra_id_99>"
        assert (min(map(len, pl["plain"])), max(map(len, pl["plain"]))) == first
        assert (min(map(len, pl["meta"])), max(map(len, pl["meta"]))) == meta
        ids = lp.new_ids(name)
        assert len(ids) == len(pl["plain"]) + len(pl["meta"]) and all(3 <= i < 32000 for i in ids.values())
        plain_now = [p for p, _ in v[3:32000] if not p.startswith(lp.META)]
        meta_now = [p[1:] for p, _ in v[3:32000] if p.startswith(lp.META)]
        assert max(len(p.encode()) for p in plain_now) == first[1]
        assert max(len(p.encode()) for p in meta_now) == meta[1]
    pl = lp.plan("v19")
    assert len(pl["plain"]) == 48 and len(pl["pairs"]) >= 4 and len(pl["pfx"]) >= 3
    for a, b in pl["pairs"]:
        assert a != b and len(a) == len(b) and a[:16] == b[:16]
    proxy = {p for p, _ in lp.build("v19")["model"]["vocab"]} - set(pl["plain"])
    for p in pl["pfx"]:  # their first 4 bytes open a shorter proxy piece too
        assert any(q.startswith(p[:4]) for q in proxy if 4 <= len(q) <= 8)


def test_oracle_matches_tokenizers_on_long_pieces(variant):
    tokenizers = pytest.importorskip("tokenizers")
    name, path = variant
    ref = tokenizers.Tokenizer.from_file(path)
    tok = oracle_lib.T5Tok(path)
    new = set(lp.new_ids(name).values())
    used, bad = 0, []
    for t in piece_texts(name):
        want = ref.encode(t).ids
        got = tok.encode(t)
        used += sum(1 for i in want if i in new)
        if got != want:
            bad.append((t[:60], want[:8], got[:8]))
    print(f"{name}: {len(bad)} of {N_TEXTS} texts differ, {used} uses of the new ids")
    assert not bad, f"{len(bad)} of {N_TEXTS} texts differ, e.g. {bad[:2]}"
    assert used > 0, "no text used a new piece"


def test_oracle_picks_every_new_piece_alone(variant):
    """A new piece as a word of its own ("▁" pieces: their payload) encodes to "▁" + the piece or
    to the "▁" piece itself, and changing a byte past the 16th loses it -- so the GPU cases built
    from the pieces do run a lattice in which a candidate longer than 16 bytes wins.  (A near miss
    hashes to other table slots than the piece; the strings of test_collision_strings are the
    ones only a compare of the bytes past 16 rejects.)"""
    name, path = variant
    tok = oracle_lib.T5Tok(path)
    ids = lp.new_ids(name)
    pl = lp.plan(name)
    for p in pl["plain"]:
        assert tok.encode(p)[1:-1] == [ids[p]], p
        near = p[:-1] + ("#" if p[-1] != "#" else "%")
        assert ids[p] not in tok.encode(near) and len(tok.encode(near)) > 3
    for m in pl["meta"]:
        assert tok.encode(m)[:-1] == [ids[lp.META + m]], m
    for a, b in pl["pairs"]:
        assert tok.encode(a) != tok.encode(b)


def test_hash_restatement_matches_the_sources():
    """The generator's piece_hash / cuckoo_slot1 / cuckoo_slot2 against values printed by
    common.hpp's ph_init, ph_mix, ph_final and slot functions over assets.cpp's block loop
    (mask 2^18 - 1)."""
    for w, h, s1, s2 in (("a", 2945481371, 31387, 60753), ("abcdefghijklmnopq", 214655847, 222055, 205937),
                         ("abcdefghijklmnopqrstuvwxyz0123456789ABCDEFGHIJKLMNOPQ", 17800506, 236858, 71041)):
        assert lp.piece_hash(w.encode()) == h
        assert (lp.cuckoo_slot1(h, 0x3FFFF), lp.cuckoo_slot2(h, 0x3FFFF)) == (s1, s2)
        assert lp.piece_slots(w.encode()) == (s1, s2)


@pytest.mark.parametrize("name", ["v19", "v32"])
def test_collision_strings(name, tmp_path_factory):
    """collisions(): each string keeps a piece's length and all but its last three bytes, one of
    its two slot indices equals one of the piece's on 18 bits (so under any table of <= 2^18
    slots), and the oracle does not find the piece in it.  For at least 8 pieces all four
    (string slot, piece slot) kinds exist: whichever slot the builder gave the piece, one string
    meets it with its first and one with its second probed slot."""
    col = lp.collisions(name)
    pl = lp.plan(name)
    ids = lp.new_ids(name)
    tok = oracle_lib.T5Tok(write_variant(tmp_path_factory, name))
    kinds = {}
    for p, s, k, j in col:
        assert p in pl["plain"] and s not in pl["plain"] and len(s) == len(p) >= 19 and s[:-3] == p[:-3] and s != p
        assert s[:16] == p[:16] and all(0x21 <= ord(c) <= 0x7E for c in s)
        assert lp.piece_slots(s.encode())[k - 1] == lp.piece_slots(p.encode())[j - 1]
        assert ids[p] not in tok.encode(s) and ids[p] in tok.encode(p)
        kinds.setdefault(p, set()).add((k, j))
    assert sum(1 for v in kinds.values() if len(v) == 4) >= 8
    # 32,100 pieces and the added tokens: the table has 2^16 .. 2^18 slots
    assert 2 * 32100 <= 1 << lp.COLLIDE_BITS


def test_host_loader_accepts_the_variants(native_lib, variant):
    from streaming_data_loader_amd import native
    name, path = variant
    info = native.tokenizer_info(path)
    assert info.kind == 2 and info.eos_id == 1 and info.unk_id == 2 and info.vocab_size == 32100


def test_host_loader_refuses_a_65_byte_piece(native_lib, tmp_path_factory):
    from streaming_data_loader_amd import native
    pl = lp.plan("too_long")
    assert [len(p) for p in pl["plain"]] == [65] and not pl["meta"]
    path = write_variant(tmp_path_factory, "too_long")
    with pytest.raises(native.SDLError, match="longer than 64 bytes"):
        native.tokenizer_info(path)
