"""The reference chain of tests/test_gpu_bpe_paths.py on the synthetic merge tables.

tests/golden/make_bpe_merge_vocab.py draws byte-level BPE tables on which random words merge over
a dozen rounds and more into many distinct ids.  The GPU cases compare the HIP kernels with
oracle/orc_bpe.c on them, so this module first pins that oracle, without any code under test:
  * to the `tokenizers` crate, id for id, on N_TEXTS seeded texts per table -- words of 2..3000
    bytes over the tables' letters, single and repeated spaces, contractions, digits, punctuation,
    letters outside the merge alphabet, the added token;
  * to the two plain models of tests/bpe_merge_model.py (tokenizers' heap order and the device's
    "every occurrence of the lowest rank" rounds) on the texts of letter-words joined by single
    spaces, whose pre-tokens are known by construction.
The number of differing texts must be 0 in every comparison.  Also here: the generator's
conditions, and the host loader's view of a table and its refusal of a non-monotone one."""
import random

import pytest

import bpe_merge_model as model
import make_bpe_merge_vocab as mv
import oracle_lib

N_TEXTS = 320
LENGTHS = (2, 3, 4, 7, 11, 12, 13, 16, 17, 24, 33, 40, 63, 64, 65, 66, 127, 128, 129, 300)
RARE_LENGTHS = (500, 1023, 1024, 1025, 1500, 3000)


@pytest.fixture(scope="module", params=mv.SEEDS)
def tab(request, tmp_path_factory):
    t = mv.table(request.param)
    return t, mv.write(request.param, str(tmp_path_factory.mktemp(f"bpe_merge_{request.param}")))


def word(rng, t, long_self):
    k = rng.randrange(12)
    if k == 0:
        return rng.choice(long_self)
    if k == 1:  # a near miss of a long self-encoding token: one tail byte changed
        w = bytearray(rng.choice(long_self))
        w[-1] = ord("a") if w[-1] != ord("a") else ord("b")
        return bytes(w) if w[-2] < 0x80 and w[-1] < 0x80 else rng.choice(long_self)
    if k == 2:  # runs of one letter: the self-pairs
        return rng.choice(mv.LETTERS[:3]) * rng.randint(2, 9) + mv.random_word(rng, rng.randint(0, 5))
    n = rng.choice(RARE_LENGTHS) if rng.random() < 0.04 else rng.choice(LENGTHS)
    return mv.random_word(rng, n)


def texts(t, n=N_TEXTS):
    """[(text bytes, word_only)]: half letter-words joined by single spaces, half mixed."""
    rng = random.Random(t.seed + 5)
    long_self = [s.lstrip(b" ") for s in t.self_encoding()]  # (after a space, " xyz" is the pre-token)
    extras = [b"'s", b"'ll", b"'t", b"'re", b"  ", b"\n", b" \n ", b"12", b"!", b"?!", b"don't", b"xyz", b"Q",
              mv.EOS.encode(), "ñ".encode(), b"\t", b"   "]
    out = []
    for i in range(n):
        ws = [word(rng, t, long_self) for _ in range(rng.randint(1, 12))]
        if i % 2 == 0:
            out.append((b" ".join(ws), True))
        else:
            s = b""
            for w in ws:
                s += w + rng.choice([b" ", b" ", b" "] + extras)
                if rng.random() < 0.3:
                    s += rng.choice(extras)
            out.append((s, False))
    return out


def test_generator_conditions():
    assert len(mv.SEEDS) >= 2
    for seed in mv.SEEDS:
        t = mv.table(seed)
        assert mv.conditions(t) is None and t.seed == seed  # (SEEDS need no re-draw: printed seeds are theirs)
        t.check_monotone()
        assert 100 <= len(t.merges) <= 300 and t.eos == 256 + len(t.merges)
        assert len(set(t.merges)) == len(t.merges) and len({l + r for l, r in t.merges}) == len(t.merges)
        assert max(len(l + r) for l, r in t.merges) <= mv.MAX_PIECE
        lens = sorted(map(len, t.self_encoding()))
        assert len(lens) >= mv.MIN_LONG_SELF and lens[0] >= 17 and 32 < lens[-1] <= 40
        assert t.merges[mv.SELF1][0] == t.merges[mv.SELF1][1] and len(t.merges[mv.SELF1][0]) == 1
        assert t.merges[mv.SELF2][0] == t.merges[mv.SELF2][1] and len(t.merges[mv.SELF2][0]) == 2
        assert any(l[0] >= 0x80 for l, r in t.merges) and any(l == b" " for l, r in t.merges)
        rng = random.Random(seed)
        for n in mv.COND_LENGTHS:
            rounds, distinct = t.rounds(mv.random_word(rng, n))
            assert rounds >= mv.MIN_ROUNDS and distinct >= mv.MIN_DISTINCT, (n, rounds, distinct)


def test_models_agree_on_self_pair_runs():
    """Odd and even runs of the self-pair letter: heap order == rounds."""
    for seed in mv.SEEDS:
        t = mv.table(seed)
        x = t.merges[mv.SELF1][0]
        for n in range(2, 40):
            for pre in (b"", b"b", b"ca"):
                w = pre + x * n + b"b"
                assert model.heap_encode(list(w), t.pair) == model.batch_encode(list(w), t.pair), w


def test_oracle_tokenizers_and_models_agree(tab):
    tokenizers = pytest.importorskip("tokenizers")
    t, path = tab
    ref = tokenizers.Tokenizer.from_file(path)
    tok = oracle_lib.Gpt2Tok(path)
    bad_ref, bad_heap, bad_batch, n_words, merged = [], [], [], 0, 0
    for s, word_only in texts(t):
        got = tok.encode(s)
        if got != ref.encode(s.decode()).ids:
            bad_ref.append(s[:60])
        merged += sum(1 for i in got if 256 <= i < t.eos)
        if word_only:
            n_words += 1
            pieces = model.split_words(s)
            heap = [i for p in pieces for i in model.heap_encode(list(p), t.pair)]
            batch = [i for p in pieces for i in model.batch_encode(list(p), t.pair)]
            if heap != got:
                bad_heap.append(s[:60])
            if batch != got:
                bad_batch.append(s[:60])
    print(f"seed {t.seed}: {len(bad_ref)} of {N_TEXTS} texts differ from tokenizers; heap model "
          f"{len(bad_heap)}, batch model {len(bad_batch)} of {n_words} word-only texts differ; "
          f"{merged} merged ids")
    assert not bad_ref, f"{len(bad_ref)} of {N_TEXTS} texts differ from tokenizers, e.g. {bad_ref[:2]}"
    assert not bad_heap, f"heap model: {len(bad_heap)} of {n_words} differ, e.g. {bad_heap[:2]}"
    assert not bad_batch, f"batch model: {len(bad_batch)} of {n_words} differ, e.g. {bad_batch[:2]}"
    assert n_words >= 150 and merged > 0


def test_models_agree_with_oracle_without_tokenizers(tab):
    """The same chain for a machine without `tokenizers`: oracle == heap == rounds on long words."""
    t, path = tab
    tok = oracle_lib.Gpt2Tok(path)
    rng = random.Random(t.seed + 9)
    for n in (2, 12, 13, 64, 65, 129, 1024, 1025, 3000):
        w = mv.random_word(rng, n)
        for p in (w, b" " + w):
            got = tok.encode(p)
            assert got == model.heap_encode(list(p), t.pair) == model.batch_encode(list(p), t.pair), (n, p[:40])


def test_host_loader_accepts_the_tables(native_lib, tab):
    from streaming_data_loader_amd import native
    t, path = tab
    info = native.tokenizer_info(path)
    assert info.eos_id == t.eos and info.vocab_size == t.eos + 1


def test_host_loader_refuses_a_non_monotone_table(native_lib, tmp_path_factory):
    """One merge moved ahead of the merge that creates its left part: the device's rounds would no
    longer be tokenizers' order, and load_byte_bpe says so."""
    from streaming_data_loader_amd import native
    path = mv.write(mv.SEEDS[0], str(tmp_path_factory.mktemp("bpe_non_monotone")), mv.non_monotone(mv.SEEDS[0]))
    with pytest.raises(native.SDLError, match="not rank-monotone"):
        native.tokenizer_info(path)
