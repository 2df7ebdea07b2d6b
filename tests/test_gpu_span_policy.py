"""GPU parity of T5's span corruption (sdl_config.span_policy 1; pipeline.hip k_rows_span_t5,
span_noise.hpp) with the Python model of the contract (span_noise_model.py): every plane of every
row, bit for bit, nothing sampled; d_label_errors is 0 everywhere.  Each case's model rows are
made once and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib
import span_noise_model as M
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_parity import run_device, torch  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 1234
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("input_ids", "attention_mask", "labels")


@functools.lru_cache(maxsize=None)
def long_records(k):
    """The fixture's records joined k at a time: records of thousands of ids, so wide rows are full."""
    recs = M.fixture_records()
    return tuple(" ".join(recs[i:i + k]) for i in range(0, len(recs), k))


@functools.lru_cache(maxsize=None)
def want(name, S, per_mille=150, mean=3.0, first_record=0, min_ids=64, lo=0, hi=None):
    texts = {"fixture": M.fixture_records, "long": lambda: long_records(12)}[name]()[lo:hi]
    planes, info = M.rows(texts, S, per_mille, mean, SEED, first_record, min_ids)
    for a in planes.values():
        a.setflags(write=False)
    return texts, planes, info


def device_planes(torch, texts, S, per_mille=150, mean=3.0, first_record=0, min_ids=64, B=8, **kw):  # noqa: F811
    db = DeviceBatcher(task=native.SDL_TASK_SPAN, batch_size=B, sequence_length=S, seed=SEED, min_ids=min_ids,
                       tokenizer=native.T5_PROXY_TOKENIZER, avg_span_size=mean, span_policy=1,
                       span_noise_per_mille=per_mille, **kw)
    res = run_device(torch, db, list(texts), first_record=first_record)
    G = res.rows()
    ids, am, tt, lab = res.planes(G + (-G) % B)
    assert tt is None and lab.shape[1] == S // 4
    assert res.label_errors() == 0 and res.tokenize_errors() == 0
    db.close()
    return {"input_ids": ids, "attention_mask": am, "labels": lab}, G


def assert_rows(got, G, wanted, what):
    assert wanted["input_ids"].shape[0] == G and G > 0, (what, wanted["input_ids"].shape, G)
    for k in KEYS:
        bad = np.nonzero((got[k][:G] != wanted[k]).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {k}, {bad.size} of {G} rows differ, first {bad[:5]}"
    # rows of the last batch nobody filled keep T5Data::new's values
    assert (got["input_ids"][G:] == 0).all() and (got["attention_mask"][G:] == 1).all()
    assert (got["labels"][G:] == -100).all()


# ---- the bulk path ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [64, 100, 128, 257, 512])
def test_bulk_rows_match_the_model(torch, native_lib, S):  # noqa: F811
    """Widths on and off the 4-int grid (16-byte and scalar stores), B = 8."""
    texts, wanted, info = want("fixture", S)
    assert max(len(i["a"]) for i in info) >= 3 and any(i["n"] == S for i in info) and any(i["n"] < S for i in info)
    got, G = device_planes(torch, texts, S)
    assert_rows(got, G, wanted, f"S={S}")


@pytest.mark.parametrize("S, per_mille", [(1024, 150), (2048, 100)])
def test_wide_rows_match_the_model(torch, native_lib, S, per_mille):  # noqa: F811
    """Full rows of 1024 ids (52 sentinels) and 2048 ids (69 sentinels; two waves a workgroup)."""
    texts, wanted, info = want("long", S, per_mille)
    assert sum(i["n"] == S for i in info) >= 4 and max(len(i["a"]) for i in info) == M.counts(S, per_mille, 3.0)[1]
    got, G = device_planes(torch, texts, S, per_mille)
    assert_rows(got, G, wanted, f"S={S}")


# ---- edge rows ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_texts(S):
    """Records whose last chunks hold 1, 2, 3 and 7 ids, exactly S and S - 1 ids, and whole records
    of 3, 4 and S - 1 ids."""
    return tuple(M.grown_record(n, seed=n) for n in (S + 1, S + 2, S + 3, S + 7, 2 * S, 2 * S - 1, 3, 4, S - 1, S))


@functools.lru_cache(maxsize=None)
def edge_want(S, per_mille, mean):
    planes, info = M.rows(edge_texts(S), S, per_mille, mean, SEED, 0, 0)
    return planes, info


@pytest.mark.parametrize("per_mille, mean, what", [
    (150, 3.0, "T5's own setting"),
    (1, 3.0, "per mille 1: one noise id a row"),
    (172, 3.0, "the densest setting S = 64 takes at mean 3.0: the full row's labels fill S/4 exactly"),
    (100, 1.0, "mean 1.0: every span is one id"),
    (150, 50.0, "a mean larger than t: one span a row"),
])
def test_edge_rows(torch, native_lib, per_mille, mean, what):  # noqa: F811
    S = 64
    wanted, info = edge_want(S, per_mille, mean)
    last = {}
    for i in info:
        last[i["rec"]] = i
    assert [last[r]["n"] for r in range(10)] == [1, 2, 3, 7, S, S - 1, 3, 4, S - 1, S]  # the last chunks
    assert last[0]["a"] == [] and last[1]["a"] == [1] and last[1]["b"] == [1]
    full = M.counts(S, per_mille, mean)
    if per_mille == 1:
        assert all(sum(i["b"]) == 1 for i in info if i["n"] > 1)
    if per_mille == 172:
        assert full[0] + full[1] + 1 == S // 4
    if mean == 1.0:
        assert full[1] == full[0] and all(set(i["b"]) <= {1} for i in info)
    if mean == 50.0:
        assert all(len(i["b"]) <= 1 for i in info)
    got, G = device_planes(torch, edge_texts(S), S, per_mille, mean, min_ids=0)
    assert_rows(got, G, wanted, what)


def test_per_mille_500_never_fits_the_label_row(torch, native_lib):  # noqa: F811
    """Half a row's ids as noise need more than S/4 labels at every S: the densest accepted word is
    below 250.  The refusal is the capacity row of the contract, with a device present."""
    for S, mean in ((64, 3.0), (512, 3.0), (2048, 2048.0)):
        assert M.capacity(S, 500, mean)[0] > S // 4
        with pytest.raises(native.SDLError) as e:
            DeviceBatcher(task=native.SDL_TASK_SPAN, sequence_length=S, tokenizer=native.T5_PROXY_TOKENIZER,
                          avg_span_size=mean, span_policy=1, span_noise_per_mille=500)
        assert e.value.code == -1 and "labels" in str(e.value)


# ---- the host interfaces ----------------------------------------------------------------------------------
def _filled(batches):
    return {k: np.concatenate([np.asarray(getattr(d, k))[:d.rows] for d in batches]) for k in KEYS}


def _drain(gt, batches):
    last = gt.get_working_batch()
    while last is not None and last.rows:
        batches.append(last)
        last = gt.get_working_batch()
    return batches


def test_per_record_pushes_and_flush_equal_the_bulk_call(torch, native_lib):  # noqa: F811
    from streaming_data_loader_amd import BatchConfig, GenTokenizer, ModelType, Span, TokenizerConfig
    S = 128
    texts, wanted, _ = want("fixture", S, 150, 3.0, 0, 64, 0, 40)
    cfg = (ModelType.T5, BatchConfig(8, S), Span(16.0, 3.0, policy=1, noise_per_mille=150),
           TokenizerConfig(native.T5_PROXY_TOKENIZER))
    one = GenTokenizer(*cfg, chunk=True, seed=SEED)
    pushed = _drain(one, [b for b in (one.create_sync_batch(t) for t in texts) if b is not None])
    bulk = GenTokenizer(*cfg, chunk=True, seed=SEED)
    ref = _drain(bulk, bulk.create_sync_batches(list(texts)))
    assert [d.rows for d in pushed] == [d.rows for d in ref] and len(pushed) > 2
    assert all(d.token_type_ids is None for d in pushed)
    got, exp = _filled(pushed), _filled(ref)
    for k in KEYS:
        np.testing.assert_array_equal(got[k], exp[k], err_msg=k)
        np.testing.assert_array_equal(got[k], wanted[k], err_msg=k)
    one.close()
    bulk.close()


@pytest.mark.parametrize("shards", [2, 3])
def test_shards_equal_one_handle(torch, native_lib, shards):  # noqa: F811
    from streaming_data_loader_amd import BatchConfig, ModelType, ShardedGenTokenizer, Span, TokenizerConfig
    S = 128
    texts, wanted, _ = want("fixture", S)
    sh = ShardedGenTokenizer(ModelType.T5, BatchConfig(8, S), Span(16.0, 3.0), TokenizerConfig(native.T5_PROXY_TOKENIZER),
                             devices=[0] * shards, seed=SEED, span_policy=1, span_noise_per_mille=150)
    per = sh.create_sync_batches(list(texts))
    got = []
    for k in range(shards):
        got += per[k]
        last = sh.get_working_batch(k)
        while last is not None and last.rows:
            got.append(last)
            last = sh.get_working_batch(k)
    assert all(len(p) > 0 for p in per)
    filled = _filled(got)
    for k in KEYS:
        np.testing.assert_array_equal(filled[k], wanted[k], err_msg=k)
    sh.close()


def test_a_record_range_keyed_by_its_global_index(torch, native_lib):  # noqa: F811
    S, a, b = 128, 7, 31
    _, wanted, info = want("fixture", S)
    keep = [g for g, i in enumerate(info) if a <= i["rec"] < b]
    got, G = device_planes(torch, M.fixture_records()[a:b], S, first_record=a)
    assert_rows(got, G, {k: wanted[k][keep] for k in KEYS}, f"records [{a}, {b})")


def test_the_same_call_twice_is_identical(torch, native_lib):  # noqa: F811
    texts = M.fixture_records()
    a, G = device_planes(torch, texts, 256)
    b, G2 = device_planes(torch, texts, 256)
    assert G == G2 and all((a[k] == b[k]).all() for k in KEYS)


CHILD = """
import sys
import numpy as np
sys.path.insert(0, {tests!r})
import torch
import span_noise_model as M
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher
from test_gpu_parity import run_device
db = DeviceBatcher(task=native.SDL_TASK_SPAN, batch_size=8, sequence_length=128, seed={seed}, tokenizer=native.T5_PROXY_TOKENIZER,
                   avg_span_size=3.0, span_policy=1, span_noise_per_mille=150)
res = run_device(torch, db, list(M.fixture_records()))
G = res.rows()
ids, am, tt, lab = res.planes(G)
np.savez({out!r}, input_ids=ids, attention_mask=am, labels=lab, errors=res.label_errors())
db.close()
"""


def test_two_phase_switch_has_no_effect(torch, native_lib, tmp_path):  # noqa: F811
    """SDL_SPAN_TWO_PHASE is read when the library loads: a fresh child process with it set gives
    the planes this process (variable unset) and the model give."""
    assert not os.environ.get("SDL_SPAN_TWO_PHASE")
    out = str(tmp_path / "two_phase.npz")
    env = dict(os.environ, SDL_SPAN_TWO_PHASE="1")
    code = CHILD.format(tests=os.path.join(REPO, "tests"), seed=SEED, out=out)
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    child = np.load(out)
    texts, wanted, _ = want("fixture", 128)
    got, G = device_planes(torch, texts, 128)
    assert int(child["errors"]) == 0
    for k in KEYS:
        np.testing.assert_array_equal(child[k], got[k][:G], err_msg=k)
        np.testing.assert_array_equal(child[k], wanted[k], err_msg=k)


def test_zeroed_policy_is_still_the_oracles_span_rows(torch, native_lib):  # noqa: F811
    from test_gpu_span import oracle_span_rows
    S, B_ = 128, 8
    blobs = [r.encode() for r in M.fixture_records()]
    db = DeviceBatcher(task=native.SDL_TASK_SPAN, batch_size=B_, sequence_length=S, seed=77,
                       tokenizer=native.T5_PROXY_TOKENIZER, span_policy=0, span_noise_per_mille=0)
    res = run_device(torch, db, blobs, first_record=5)
    G = res.rows()
    ids, am, tt, lab = res.planes(G + (-G) % B_)
    wanted, errs = oracle_span_rows(M.tok(), blobs, B_, S, 77, first_record=5)
    assert G == wanted["input_ids"].shape[0]
    np.testing.assert_array_equal(ids[:G], wanted["input_ids"])
    np.testing.assert_array_equal(am[:G], wanted["attention_mask"])
    np.testing.assert_array_equal(lab[:G], wanted["labels"])
    assert res.label_errors() == errs and (am == 1).all()
    db.close()


def test_pickle_frames_of_a_policy_batch(torch, native_lib):  # noqa: F811
    """The transport frames carry the policy's planes: each equals the oracle's serde_pickle of the
    model's batch (the partial last one with its unfilled rows at the initial values)."""
    S, Bsz = 128, 8
    texts, wanted, _ = want("fixture", S)
    full = M.padded(wanted, Bsz)
    db = DeviceBatcher(task=native.SDL_TASK_SPAN, batch_size=Bsz, sequence_length=S, seed=SEED,
                       tokenizer=native.T5_PROXY_TOKENIZER, avg_span_size=3.0, span_policy=1, span_noise_per_mille=150)
    res = run_device(torch, db, list(texts))
    G = res.rows()
    assert G == wanted["input_ids"].shape[0] and G % Bsz != 0
    frames = db.pickle_frames(res, G, flush_partial=True).frames()
    assert len(frames) == -(-G // Bsz)
    for f, frame in enumerate(frames):
        sl = slice(f * Bsz, (f + 1) * Bsz)
        ref = oracle_lib.pickle_dataset("span", Bsz, S, S // 4, min(Bsz, G - f * Bsz), full["input_ids"][sl],
                                        full["attention_mask"][sl], None, full["labels"][sl])
        assert frame == ref, f
    db.close()
