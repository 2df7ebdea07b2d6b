"""The BERT masking policies without a GPU: the Python model of the contract (mlm_policy_model.py)
against the issue's known answers and its invariants, the C ABI's new fields and argument checks
(which return before a device is looked for), and the whole-word pick of csrc/mlm_pick.hpp in a
stand-alone host program against the contract's own sort, forced equal keys included."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import mlm_policy_model as M
import oracle_lib
from test_list_index import CSRC, HERE, host_compiler

SEED = 1234


def test_model_philox_is_the_oracles():
    for rec, chunk in ((0, 0), (7, 3), (1 << 33, 1)):
        w = M.row_words(SEED, rec, chunk, 130)
        for pos in (0, 1, 2, 3, 4, 63, 127, 129):
            assert int(w[pos]) == oracle_lib.lib().orc_mlm_key(SEED, rec, chunk, pos)


@functools.lru_cache(maxsize=None)
def fixture_rows():
    import json
    with open(os.path.join(HERE, "golden", "test_records.jsonl"), encoding="utf-8") as f:
        recs = [json.loads(l)["text"] for l in f]
    rows, where = M.unmasked_rows(recs, 128, min_ids=64)
    rows.setflags(write=False)
    return rows, where


@functools.lru_cache(maxsize=None)
def fixture_masked(policy):
    rows, where = fixture_rows()
    return M.apply(rows, where, policy, SEED, 19, 150, 103)


def test_known_answers_rows_and_first_row():
    """Proxy vocabulary, the fixture's records, S=128, seed 1234, mask_length 19, 150 per mille,
    mask_id 103, min_ids 64: 182 rows; row 0 (record 0, chunk 0, l = 128) picks the issue's 19
    positions; policies 1 and 2 pick the same positions on this corpus."""
    vocab_size, cont, cls, sep = M.proxy_vocab()
    assert (vocab_size, int(cont.sum()), cls, sep) == (30522, 6879, 101, 102)
    rows, where = fixture_rows()
    assert rows.shape == (4, 182, 128) and where[0] == (0, 0, 128)
    got1, info1 = fixture_masked(1)
    got2, info2 = fixture_masked(2)
    assert info1[0]["sel"] == [5, 7, 13, 16, 18, 35, 36, 37, 40, 48, 55, 61, 87, 95, 111, 114, 117, 124, 126]
    assert [i["sel"] for i in info1] == [i["sel"] for i in info2]
    assert (got1 == got2).all()


def test_known_answers_totals():
    """The issue's totals over the 182 rows: 3,024 selected positions, of which 2,438 become
    mask_id, 297 a random id and 289 stay."""
    rows, _ = fixture_rows()
    got, info = fixture_masked(1)
    picked = got[3] != -100
    n_sel = sum(len(i["sel"]) for i in info)
    assert int(picked.sum()) == n_sel
    u_mask = int(((got[0] == 103) & picked).sum())
    stay = int(((got[0] == rows[0]) & picked).sum())
    print("selected", n_sel, "mask_id", u_mask, "random", n_sel - u_mask - stay, "stay", stay)
    assert (n_sel, u_mask, n_sel - u_mask - stay, stay) == (3024, 2438, 297, 289)


@functools.lru_cache(maxsize=None)
def synthetic(S):
    rows, where = M.unmasked_rows(M.synthetic_texts(), S, min_ids=0)
    rows.setflags(write=False)
    return rows, where


@pytest.mark.parametrize("S", [64, 128, 512])
def test_properties_on_synthetic_text(S):
    rows, where = synthetic(S)
    mask_length = int(np.float32(S) * np.float32(0.15))
    _, cont, cls, sep = M.proxy_vocab()
    excluded = {0, 103, cls, sep}
    assert any(cont[int(rows[0, g, 0])] for g in range(len(where))), "no row starts inside a word"
    skipped = below = nothing = 0
    for policy in (1, 2):
        got, infos = M.apply(rows, where, policy, SEED, mask_length)
        for g, info in enumerate(infos):
            sel = set(info["sel"])
            assert all(int(rows[0, g, j]) not in excluded and j < where[g][2] for j in sel)
            assert info["taken"] == len(sel) <= info["k"] <= mask_length
            assert ((got[3, g] != -100) == np.isin(np.arange(S), list(sel))).all()
            assert (got[1:3, g] == rows[1:3, g]).all()
            for u in info["units"]:
                assert sel.issuperset(u) or sel.isdisjoint(u)
                if policy == 1:
                    assert len(u) == 1
            if policy == 1:  # the k smallest keys among the candidates, all of them if fewer
                assert len(sel) == min(info["k"], len(info["units"]))
            else:
                skipped += info["skipped"]
                below += info["taken"] < info["k"]
                nothing += info["k"] > 0 and not sel
    print(f"S={S}: skipped units {skipped}, rows ending below k {below}, rows that select nothing {nothing}")
    # preconditions: the inputs are such that the skip rule acts
    assert skipped > 0 and below > 0 and nothing > 0, (skipped, below, nothing)


# ---- the C ABI: additive fields, checks before the device lookup -------------------------------
def create_rc(native_lib, tokenizer=None, **fields):
    from streaming_data_loader_amd import native
    c = native.default_config(fields.pop("task", native.SDL_TASK_MLM))
    for k, v in fields.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), (tokenizer or native.BERT_PROXY_TOKENIZER).encode(),
                                       native.DATA_DIR.encode(), ctypes.byref(h))
    if h:
        native_lib.sdl_batcher_destroy(h)
    return rc, native_lib.sdl_last_error().decode()


def test_config_struct_keeps_its_size_and_gains_two_fields(native_lib):
    from streaming_data_loader_amd import native
    assert ctypes.sizeof(native.Config) == 96
    assert native.Config.mask_policy.offset == 72 and native.Config.mask_per_mille.offset == 76
    assert native.Config.reserved.size == 16
    assert (native.SDL_MASK_REFERENCE, native.SDL_MASK_BERT, native.SDL_MASK_BERT_WHOLE_WORD) == (0, 1, 2)
    for task in range(5):
        c = native.default_config(task)
        assert (c.mask_policy, c.mask_per_mille) == (0, 150) and list(c.reserved) == [0, 0, 0, 0]


@pytest.mark.parametrize("fields, code", [
    (dict(mask_policy=3), -1), (dict(mask_policy=-1), -1),
    (dict(mask_policy=1, task=1), -1), (dict(mask_policy=2, task=3), -1),
    (dict(mask_policy=1, mask_per_mille=0), -1), (dict(mask_policy=2, mask_per_mille=1001), -1),
    (dict(mask_policy=1, rng_mode=1), -4), (dict(mask_policy=2, rng_mode=1), -4),
])
def test_create_checks_the_policy_before_it_looks_for_a_device(native_lib, fields, code):
    """SDL_ERR_ARG (-1) / SDL_ERR_UNSUPPORTED (-4), with or without a GPU (never SDL_ERR_NODEV)."""
    rc, msg = create_rc(native_lib, **fields)
    assert rc == code, (rc, msg)
    assert "mask_p" in msg


def test_mask_per_mille_is_ignored_under_the_reference_policy(native_lib):
    """Zeroed new fields are today's behaviour: no argument error (no device here: SDL_ERR_NODEV)."""
    rc, msg = create_rc(native_lib, mask_policy=0, mask_per_mille=0)
    assert rc in (0, -5), (rc, msg)


# ---- the pick's selection logic, on the host ----------------------------------------------------
def test_pick_units_against_the_contracts_sort(tmp_path):
    exe = str(tmp_path / "mlm_pick_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "mlm_pick_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mlm_pick ok" in r.stdout
