"""tests/uni_census.py: its constants come from the kernel sources, and its classification of a
few hand-counted chunks is what tokenize_unigram.hip's chunk kernel does with them."""
import json

import numpy as np
import pytest

import oracle_lib
import uni_census


@pytest.fixture(scope="module")
def census():
    with open(oracle_lib.T5_JSON, encoding="utf-8") as f:
        return uni_census.Census(json.load(f)["model"]["vocab"])


def test_constants_are_read_from_the_sources():
    """Every constant the census uses is an integer literal in common.hpp / tokenize_unigram.hip
    (a renamed or derived one fails here, not by testing the wrong side of a limit), and the
    relations the GPU cases rely on hold."""
    K = uni_census.constants()
    assert set(K) == set(uni_census.NAMES)
    assert all(isinstance(v, int) and v > 0 for v in K.values())
    assert K["CHUNK"] == 1024  # records of 1,024 bytes are the chunks of test_gpu_unigram_paths.py
    assert K["UNI_WMAX"] < K["UNI_VMAX"] < K["CHUNK"] and K["UNI_VMAX"] <= 63
    assert K["ARENA"] % K["UNI_WMAX"] == 0 and K["ARENA"] // K["UNI_WMAX"] < K["MED_CAP"]
    assert K["LONG_NORM1"] < K["LONG_NORM"] <= K["LONG_RAW"]
    assert K["PFX_JOBS"] < K["UNI_VPC"]


def test_a_missing_constant_is_an_error(monkeypatch):
    monkeypatch.setattr(uni_census, "NAMES", uni_census.NAMES + ("UNI_NO_SUCH_LIMIT",))
    with pytest.raises(ValueError, match="UNI_NO_SUCH_LIMIT"):
        uni_census.constants()


def test_proxy_vocabulary_facts(census):
    assert census.maxlen_first == 16 and census.maxlen_meta == 15 and census.wide_ok
    assert census.in_word_table("the") and census.in_word_table("the,") and census.in_word_table("the.")
    assert census.clear_miss("qzxv") and not census.in_word_table("qzxv")
    assert not census.clear_miss("the") and not census.clear_miss("Qzxv") and not census.clear_miss("qz.")
    assert b"<extra_id_7>" in census.added and b"</s>" in census.added


def _one(census, text, recs=None):
    b = text.encode() if isinstance(text, str) else text
    offs = np.array(recs or [0, len(b)], np.uint64)
    return census.chunks(np.frombuffer(b, np.uint8), offs)


def test_classification(census):
    c = _one(census, "the qzxv the, " + "q" * 16 + " " + "q" * 17 + " " + "q" * 48 + " " + "q" * 49 +
             " é naïve \x7fab <extra_id_3>qzv " + "q" * 20 + "\x1f")[0]
    assert c["hits"] == 2 and c["added"] == 1
    assert c["narrow"] == 3  # qzxv, q*16, qzv
    assert c["wide"] == 2 and c["wide_lens"] == [17, 48] and c["units"] == 3 + 2 + 3
    assert c["medium"] == 3  # é, naïve, \x7fab
    assert c["long"] == 2    # q*49; 20 printable bytes and a control byte


def test_window_edge_and_record_edges(census):
    K = census.K
    # a 40-byte word whose end is the last one the window shows, then one byte later
    lim = K["CHUNK"] + K["HALO_R"] - 8
    for end, kind in ((lim - 1, "wide"), (lim, "long")):
        start = end - 40
        text = " " * start + "q" * 40 + " " + "the " * 300
        cs = _one(census, text)
        assert len(cs) >= 2 and start < K["CHUNK"]
        assert cs[0][kind] == 1 and cs[0]["wide" if kind == "long" else "long"] == 0
    # record edges cut words; an added token does not cross one
    cs = _one(census, "qzxvqzxv<extra_id_3>", recs=[0, 4, 14, 20])
    assert cs[0]["narrow"] == 3 and cs[0]["added"] == 0
    # words belong to the chunk they start in
    cs = _one(census, " " * 1020 + "qzxvqzxv the")
    assert cs[0]["narrow"] == 1 and cs[1]["narrow"] == 0 and cs[1]["hits"] == 1


def test_no_wide_jobs_without_wide_ok(census):
    vocab = [["<pad>", 0.0], ["</s>", 0.0], ["<unk>", 0.0], ["x" * 20, -8.0], ["▁a", -3.0]]
    c2 = uni_census.Census(vocab, census.K)
    assert not c2.wide_ok
    c = c2.chunks(np.frombuffer(b"q" * 17 + b" a", np.uint8), np.array([0, 19], np.uint64))[0]
    assert c["wide"] == 0 and c["long"] == 1 and c["hits"] == 1
