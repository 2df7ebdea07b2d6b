"""tests/bpe_census.py: its constants come from the kernel sources, and its classification of a
few hand-counted chunks is what tokenize_bpe.hip's chunk kernel does with them."""
import numpy as np
import pytest

import bpe_census
import make_bpe_merge_vocab as mv


@pytest.fixture(scope="module")
def census():
    t = mv.table(mv.SEEDS[0])
    return bpe_census.Census(t.is_self, t.encode_word), t


def test_constants_are_read_from_the_sources():
    K = bpe_census.constants()
    assert set(K) == set(bpe_census.NAMES)
    assert all(isinstance(v, int) and v > 0 for v in K.values())
    assert K["CHUNK"] == 1024  # records of 1,024 bytes are the chunks of test_gpu_bpe_paths.py
    assert K["WIN"] == K["HALO_L"] + K["CHUNK"] + K["HALO_R"] and K["STAGE"] >= K["CHUNK"]
    assert 2 <= K["LANE_BPE"] < K["BPE_MAX_WAVE"] == 64 < K["LONG_LDS"]
    assert K["HALO_R"] > 8 and 2 * K["WIN"] // 4 < K["CHUNK"]  # a chunk can pass the packed copy-out's room


def test_a_missing_constant_is_an_error(monkeypatch):
    monkeypatch.setattr(bpe_census, "NAMES", bpe_census.NAMES + ("BPE_NO_SUCH_LIMIT",))
    with pytest.raises(ValueError, match="BPE_NO_SUCH_LIMIT"):
        bpe_census.constants()


def _one(cs, text, recs=None):
    offs = np.array(recs or [0, len(text)], np.uint64)
    return cs.chunks(np.frombuffer(text, np.uint8), offs)


def test_classification(census):
    cs, t = census
    K = cs.K
    hit = next(s for s in t.self_encoding() if not s.startswith(b" "))
    w = lambda n: b"x" * (n - 1)  # x: outside the merge alphabet, one id a byte; with its space: n bytes
    text = hit + b"".join(b" " + w(n) for n in (12, 13, 64, 65, 2)) + b" "
    c = _one(cs, text)[0]
    assert [p[2] for p in c["pieces"]] == ["hit", "lane", "wave", "wave", "long_lds", "lane", "hit"]
    assert [p[1] for p in c["pieces"]] == [len(hit), 12, 13, 64, 65, 2, 1]
    assert c["packs"] == [[13], [64]] and list(c["form"].values()) == ["lds"]
    assert c["ids"] == 1 + 12 + 13 + 64 + 65 + 2 + 1 and c["entries"] == c["ids"] - 65 + 1
    c = _one(cs, b"x" * (K["LONG_LDS"] + 1) + b" " + b"x" * K["LONG_LDS"])
    assert c[0]["pieces"] == [(0, K["LONG_LDS"] + 1, "long_global")] and c[0]["form"] == {0: "global"}
    assert c[1]["pieces"] == [(K["LONG_LDS"] + 1, K["LONG_LDS"] + 1, "long_global")]
    assert len(c) == 3 and c[2]["pieces"] == []


def test_packing(census):
    cs, _ = census
    w = lambda n: b"x" * (n - 1)  # with its space: n bytes
    text = b"x" + b"".join(b" " + w(n) for n in (16, 16, 16, 16, 32, 32, 13, 13, 13, 13, 13, 52, 12, 20, 64, 63))
    c = _one(cs, text)[0]
    assert c["packs"] == [[16, 16, 16, 16], [32, 32], [13, 13, 13, 13], [13], [52], [20], [64], [63]]
    # (13 + 52 > 64 ends a packing; the 12 is the lane path's; 52 + 20 > 64)
    assert [p[2] for p in c["pieces"]].count("lane") == 1


def test_window_edge_and_record_edges(census):
    cs, _ = census
    K = cs.K
    lim = K["CHUNK"] + K["HALO_R"] - 8
    for end, path in ((lim - 1, "wave"), (lim, "past")):
        start = K["CHUNK"] - 10
        text = b"x " * (start // 2) + b"y" * (end - start) + b" x" * 300
        cs_ = _one(cs, text)
        assert cs_[0]["pieces"][-1] == (start - 1, end - start + 1, path)
        assert (cs_[0]["form"] == {start - 1: "lds"}) == (path == "past")
    # a record edge cuts a word; the space that ends a record is a piece of its own
    c = _one(cs, b"xyxyxyxy x ", recs=[0, 4, 11])[0]
    assert [(p[0], p[1]) for p in c["pieces"]] == [(0, 4), (4, 4), (8, 2), (10, 1)]
    # a piece ending exactly at c1 shows; pieces belong to the chunk they start in
    text = b"x " * ((K["CHUNK"] - 40) // 2) + b"y" * 40 + b" xyxy"
    c = _one(cs, text)
    assert c[0]["pieces"][-1][1:] == (41, "wave") and c[1]["pieces"] == [(K["CHUNK"], 5, "lane")]
    with pytest.raises(ValueError):
        _one(cs, b"x  y")
    with pytest.raises(ValueError):
        _one(cs, b"x 1")


def test_count_paths(census):
    cs, _ = census
    acc = bpe_census.count_paths(_one(cs, b"xy " + b"x" * 70 + b" "))  # (the record's last space: one byte symbol)
    assert acc == {"lane": 1, "long_lds": 1, "hit": 1}
