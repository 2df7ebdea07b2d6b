"""GPU parity of the BERT masking policies (sdl_config.mask_policy 1 / 2; pipeline.hip
k_rows_policy, rows_device.hpp row_policy_one, mlm_pick.hpp) with the Python model of the contract
(mlm_policy_model.py): every row of all four planes, bit for bit, nothing sampled.  The unmasked
rows are the CPU oracle's (mask_length 0); each arena's are made once and shared."""
import functools
import pickle
import random

import numpy as np
import pytest

import mlm_policy_model as M
import oracle_lib
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_parity import run_device, torch  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 1234
CHUNK = 1024
LONG_A, LONG_B = "zqxjkvzqxjkvzqxjkv", "qzvxkjwqzvxkjw"  # 15 and 9 pieces in the proxy vocabulary


def mask_length_of(S):
    return int(np.float32(S) * np.float32(0.15))


def nbytes(texts):
    return sum(len(t.encode("utf-8")) for t in texts)


# ---- arenas ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_texts():
    """The synthetic text, cut to under 60 KiB: fewer than 64 chunks, the small-call path."""
    texts, out = M.synthetic_texts(), []
    for t in texts[:-1]:
        if nbytes(out) + len(t) > (58 << 10):
            break
        out.append(t)
    out.append(texts[-1])
    assert nbytes(out) < (60 << 10) and -(-nbytes(out) // CHUNK) < 64
    return tuple(out)


@functools.lru_cache(maxsize=None)
def large_texts():
    """100-400 KiB of the same kind of text (more than 64 chunks: rows from the chunk lists), with
    one run of more than 64 KiB of whitespace inside a record."""
    rng = random.Random(23)
    texts = list(M.synthetic_texts(seed=9, n=30, lo=100, hi=500))
    ws = "".join(rng.choice(" \n") for _ in range(70 << 10))
    texts.insert(7, texts[3][:900] + ws + texts[4][:2000])
    n = nbytes(texts)
    assert (100 << 10) <= n <= (400 << 10) and -(-n // CHUNK) > 64, n
    return tuple(texts)


def edge_texts(S):
    """Records for the edge rows at sequence length S (each asserted present by the test)."""
    return ("",                                             # a row with no candidate
            LONG_A + " " + LONG_B,                          # every unit larger than k (S = 64: k = 4)
            "the " * (S - 4),                               # S + 1 framed ids: a last chunk of one id
            "a [SEP] b [MASK] c [CLS] d " * 6,              # literal specials in the text
            "the " * (S - 5) + LONG_A + " the" * 20,        # a word straddling two rows
            " ".join(M.COMMON))


@functools.lru_cache(maxsize=None)
def unmasked(name, S, min_ids, lo=0, hi=None):
    texts = {"small": small_texts, "large": large_texts}[name]() if name in ("small", "large") else edge_texts(S)
    rows, where = M.unmasked_rows(list(texts[lo:hi]), S, min_ids=min_ids)
    rows.setflags(write=False)
    return texts[lo:hi], rows, where


@functools.lru_cache(maxsize=None)
def want(name, S, policy, min_ids=0, mask_length=None, per_mille=150, first_record=0, lo=0, hi=None):
    _, rows, where = unmasked(name, S, min_ids, lo, hi)
    got, infos = M.apply(rows, where, policy, SEED, mask_length_of(S) if mask_length is None else mask_length,
                         per_mille, 103, first_record)
    got.setflags(write=False)
    return got, infos


def device_planes(torch, texts, S, policy, min_ids=0, mask_length=None, per_mille=150, first_record=0, B=16):  # noqa: F811
    db = DeviceBatcher(batch_size=B, sequence_length=S, seed=SEED, min_ids=min_ids, mask_policy=policy,
                       mask_per_mille=per_mille, mask_length=mask_length_of(S) if mask_length is None else mask_length)
    res = run_device(torch, db, list(texts), first_record=first_record)
    G = res.rows()
    Gp = -(-G // B) * B
    planes = np.stack(res.planes(Gp))
    db.close()
    return planes, G


def assert_rows(got, G, wanted, what):
    assert wanted.shape[1] == G and G > 0, (what, wanted.shape, G)
    for p, plane in enumerate(("input_ids", "attention_mask", "token_type_ids", "labels")):
        bad = np.nonzero((got[p, :G] != wanted[p]).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {plane}, {bad.size} of {G} rows differ, first {bad[:5]}"
    pad = got[:, G:]
    assert (pad[0] == 0).all() and (pad[1] == 1).all() and (pad[2] == 0).all() and (pad[3] == -100).all()


# ---- the two paths, every MR instantiation ----------------------------------------------------------
@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("S", [64, 65, 66, 100, 127, 128, 256, 257, 320, 512, 1023, 1024, 2048])
def test_small_call_path(torch, native_lib, S, policy):  # noqa: F811
    texts, _, _ = unmasked("small", S, 0)
    wanted, infos = want("small", S, policy)
    assert any(i["sel"] for i in infos)
    got, G = device_planes(torch, texts, S, policy)
    assert_rows(got, G, wanted, f"small S={S} policy {policy}")


@pytest.mark.parametrize("policy", [1, 2])
# (1024 / 2048: the MR 4 / 8 instantiations over lists; 254 / 1025 / 2047: the scalar stores, S & 3 = 2 / 1 / 3)
@pytest.mark.parametrize("S", [128, 254, 512, 1024, 1025, 2047, 2048])
def test_list_path(torch, native_lib, S, policy):  # noqa: F811
    texts, _, _ = unmasked("large", S, 0)
    wanted, infos = want("large", S, policy)
    if policy == 2:  # the skip rule acts on this text
        assert sum(i["skipped"] for i in infos) > 0 and any(len(u) > 1 for i in infos for u in i["units"])
    got, G = device_planes(torch, texts, S, policy)
    assert_rows(got, G, wanted, f"lists S={S} policy {policy}")


# ---- edge rows --------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", [1, 2])
def test_edge_rows(torch, native_lib, policy):  # noqa: F811
    S = 64
    texts, rows, where = unmasked("edge", S, 0)
    wanted, infos = want("edge", S, policy)
    _, cont, cls, sep = M.proxy_vocab()
    by_rec = {}
    for g, (r, c, l) in enumerate(where):
        by_rec.setdefault(r, []).append(g)
    g0 = by_rec[0][0]  # the empty record: framing only, k = 0, nothing changes
    assert where[g0][2] == 5 and infos[g0]["k"] == 0 and (wanted[:, g0] == rows[:, g0]).all()
    g1 = by_rec[1][0]  # two units of 15 and 9 pieces against k = 4
    if policy == 2:
        assert sorted(len(u) for u in infos[g1]["units"]) == [9, 15] and infos[g1]["k"] == 4
        assert not infos[g1]["sel"] and infos[g1]["skipped"] == 2
    assert where[by_rec[2][-1]] == (2, 1, 1) and infos[by_rec[2][-1]]["k"] == 0  # a last chunk of one id
    spec = rows[0, by_rec[3]]
    for sid in (cls, sep, 103):  # literal specials inside the text, never picked
        inner = spec[:, 2:][spec[:, 2:] == sid]
        assert inner.size >= 6
    for g in by_rec[3]:
        assert all(int(rows[0, g, j]) not in (cls, sep, 103) for j in infos[g]["sel"])
    assert cont[int(rows[0, by_rec[4][1], 0])]  # the second row of record 4 starts inside a word
    got, G = device_planes(torch, texts, S, policy)
    assert_rows(got, G, wanted, f"edge policy {policy}")


@pytest.mark.parametrize("per_mille, mask_length", [(1, None), (1000, None), (150, 0)])
@pytest.mark.parametrize("policy", [1, 2])
def test_per_mille_extremes_and_no_budget(torch, native_lib, policy, per_mille, mask_length):  # noqa: F811
    S = 128
    texts, rows, _ = unmasked("small", S, 0)
    wanted, infos = want("small", S, policy, 0, mask_length, per_mille)
    if mask_length == 0:
        assert (wanted == rows).all()
    else:
        assert max(i["k"] for i in infos) == (1 if per_mille == 1 else mask_length_of(S))
    got, G = device_planes(torch, texts, S, policy, mask_length=mask_length, per_mille=per_mille)
    assert_rows(got, G, wanted, f"per mille {per_mille} mask_length {mask_length} policy {policy}")


# ---- the host interfaces ----------------------------------------------------------------------------
def _filled(batches):
    keys = ("input_ids", "attention_mask", "token_type_ids", "labels")
    return np.stack([np.concatenate([np.asarray(getattr(d, k))[:d.rows] for d in batches]) for k in keys])


def _drain(gt, batches):
    last = gt.get_working_batch()
    while last is not None and last.rows:
        batches.append(last)
        last = gt.get_working_batch()
    return batches


@pytest.mark.parametrize("policy", [1, 2])
def test_per_record_push_equals_the_bulk_call(torch, native_lib, policy):  # noqa: F811
    """GenTokenizer record by record (the fused small-push tails are bypassed under a policy)
    against one bulk call and the model."""
    from streaming_data_loader_amd import BatchConfig, GenTokenizer, Mask, ModelType, TokenizerConfig
    S = 128
    texts = small_texts()[:24]
    cfg = (ModelType.Bert, BatchConfig(8, S), Mask(19, 103, policy, 150), TokenizerConfig())
    one = GenTokenizer(*cfg, chunk=True, seed=SEED)
    pushed = _drain(one, [b for b in (one.create_sync_batch(t) for t in texts) if b is not None])
    bulk = GenTokenizer(*cfg, chunk=True, seed=SEED)
    ref = _drain(bulk, bulk.create_sync_batches(list(texts)))
    assert [d.rows for d in pushed] == [d.rows for d in ref]
    got, exp = _filled(pushed), _filled(ref)
    np.testing.assert_array_equal(got, exp)
    wanted, _ = want("small", S, policy, 64, 19, 150, 0, 0, 24)
    np.testing.assert_array_equal(got, wanted)
    one.close()
    bulk.close()


@pytest.mark.parametrize("policy", [1, 2])
def test_sharding_invariance(torch, native_lib, policy):  # noqa: F811
    """Records [a, b) with first_record = a give the same rows as the whole stream's."""
    S, a, b = 128, 5, 17
    texts, _, where = unmasked("large", S, 64)
    wanted, _ = want("large", S, policy, 64)
    keep = [g for g, (r, _, _) in enumerate(where) if a <= r < b]
    got, G = device_planes(torch, texts[a:b], S, policy, min_ids=64, first_record=a)
    assert_rows(got, G, wanted[:, keep], f"records [{a}, {b}) policy {policy}")


def test_sharded_gen_tokenizer_matches_the_model(torch, native_lib):  # noqa: F811
    from streaming_data_loader_amd import BatchConfig, Mask, ModelType, ShardedGenTokenizer, TokenizerConfig
    S = 128
    texts, _, _ = unmasked("large", S, 64)
    wanted, _ = want("large", S, 2, 64, 19)
    sh = ShardedGenTokenizer(ModelType.Bert, BatchConfig(8, S), Mask(19, 103), TokenizerConfig(), devices=[0, 0, 0],
                             seed=SEED, mask_policy=2, mask_per_mille=150)
    per = sh.create_sync_batches(list(texts))
    got = []
    for k in range(3):
        got += per[k]
        last = sh.get_working_batch(k)
        while last is not None and last.rows:
            got.append(last)
            last = sh.get_working_batch(k)
    assert all(len(p) > 0 for p in per)
    np.testing.assert_array_equal(_filled(got), wanted)
    sh.close()


@pytest.mark.parametrize("policy", [1, 2])
def test_the_same_call_twice_is_identical(torch, native_lib, policy):  # noqa: F811
    texts = small_texts()
    a, G = device_planes(torch, texts, 256, policy)
    b, G2 = device_planes(torch, texts, 256, policy)
    assert G == G2 and (a == b).all()


def test_reference_policy_with_zeroed_fields_is_the_oracle(torch, native_lib, oracle_tok):  # noqa: F811
    S = 128
    texts = list(small_texts())
    wanted = oracle_lib.oracle_rows(oracle_tok, texts, S, 19, 103, seed=SEED, B=16)
    db = DeviceBatcher(batch_size=16, sequence_length=S, seed=SEED, mask_length=19, mask_policy=0, mask_per_mille=0)
    res = run_device(torch, db, texts)
    G = res.rows()
    assert_rows(np.stack(res.planes(-(-G // 16) * 16)), G, wanted, "policy 0")
    db.close()


# ---- refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gpt2", "t5"])
def test_whole_words_need_wordpiece(torch, native_lib, name):  # noqa: F811
    tokenizer = {"gpt2": native.GPT2_PROXY_TOKENIZER, "t5": native.T5_PROXY_TOKENIZER}[name]
    with pytest.raises(native.SDLError) as e:
        DeviceBatcher(tokenizer=tokenizer, mask_policy=2)
    assert e.value.code == -4 and "SDL_MASK_BERT_WHOLE_WORD" in str(e.value)


def test_rng_mode_1_has_no_policy(torch, native_lib):  # noqa: F811
    with pytest.raises(native.SDLError) as e:
        DeviceBatcher(mask_policy=1, rng_mode=1)
    assert e.value.code == -4 and "rng_mode" in str(e.value)


# ---- the transport frames carry the policy's planes --------------------------------------------------
def test_pickle_frames_of_a_policy_result(torch, native_lib):  # noqa: F811
    S, Bsz = 128, 16
    texts, _, _ = unmasked("small", S, 0)
    wanted, _ = want("small", S, 1)
    db = DeviceBatcher(batch_size=Bsz, sequence_length=S, seed=SEED, min_ids=0, mask_policy=1, mask_length=19)
    res = run_device(torch, db, list(texts))
    G = res.rows()
    frames = db.pickle_frames(res, G, flush_partial=True).frames()
    assert len(frames) == -(-G // Bsz)
    for f, frame in enumerate(frames):
        d = pickle.loads(frame)
        n = min(Bsz, G - f * Bsz)
        for p, key in enumerate(("input_ids", "attention_mask", "token_type_ids")):
            assert np.array_equal(np.asarray(d[key], np.int32)[:n], wanted[p, f * Bsz:f * Bsz + n]), (f, key)
        assert np.array_equal(np.asarray(d["labels"], np.int32), wanted[3, f * Bsz:f * Bsz + n]), f
    db.close()
