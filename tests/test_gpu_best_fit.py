"""Best-fit rows of a packed clm handle (sdl_batcher_set_best_fit, pack_bestfit.hip): all four planes,
*d_rows and d_record_rows, exactly, against the plain model of the contract (tests/best_fit_model.py,
include/sdl_batcher.h "Best-fit rows") over the oracle tokenizer's ids per record."""
import ctypes

import numpy as np
import pytest

import best_fit_model
import pack_model
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher
from test_gpu_pack import check, check_padding, four, run

pytestmark = pytest.mark.gpu
NAMES = ("input_ids", "attention_mask", "labels", "position_ids")
# ids per crafted record (S = 64; searched with the model): an exact fit, a tie the most-recent rule
# decides differently, a row of five pieces; a window of dropped records; segments of S, S + 1 and
# 2 S + 3 ids in a short last window of W = 8
CRAFTED = [1, 31, 48, 8, 11, 33, 20, 16] + [0] * 8
# S = 4096: a tail that leaves room 65, three rows of room 95 (a tie) and enough two-id tails to open
# a row whose room lies in the top word of the map and which holds more than 64 pieces
LONG = [4030, 4000, 4000, 4000] + [1] * 260


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def corpus(records, oracle_gpt2):
    """(blobs, ids per record, eos): the fixture records between hand-made ones of 1, 2 and 3 ids and
    empty ones."""
    small = [b"a", b"a b", b"a b c", b""]
    blobs = small + [t.encode("utf-8") for t in records] + small[::-1]
    ids = [oracle_gpt2.encode(b) for b in blobs]
    assert [len(t) for t in ids[:4]] == [1, 2, 3, 0]
    return blobs, ids, native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id


def packer(S, W, min_ids=0):
    return DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=S, min_ids=min_ids,
                         tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1, best_fit=B.BestFit(W))


def res_rows(res, torch):
    torch.cuda.synchronize()
    return res.rows()


def one_call(torch, db, blobs, ids, S, W, eos, what):
    want = best_fit_model.pack(ids, S, eos, W)
    res = run(torch, db, blobs)
    G = want[0].shape[0]
    assert res.rows() == G and res.r.rows_capacity >= -(-G // 4) * 4
    check(four(res), want[:4], what)
    check_padding(res, G, 4, S)
    np.testing.assert_array_equal(res.record_rows(), pack_model.record_rows(ids, 0))
    return want


@pytest.mark.parametrize("W", [1, 7, 64, 4096])
@pytest.mark.parametrize("S", [30, 33, 64, 65])
def test_fixture_corpus(torch, native_lib, corpus, S, W):
    blobs, ids, eos = corpus
    db = packer(S, W)
    want = one_call(torch, db, blobs, ids, S, W, eos, f"S={S} W={W}")
    assert want[0].shape[0] > len(ids) and max(map(len, ids)) > 3 * S  # many full rows and a tail each
    assert res_rows(db.flush_device(), torch) == 0  # no carry: the flush emits nothing
    db.close()


@pytest.mark.parametrize("S,W", [(64, 4096), (64, 8), (4096, 4096)])
def test_crafted_corpus(torch, native_lib, oracle_gpt2, S, W):
    counts = CRAFTED + [S - 1, S, 2 * S + 2, 5, 4] + (LONG if S == 4096 else [])
    blobs = [b"a" + b" a" * (n - 1) if n else b"" for n in counts]
    ids = [oracle_gpt2.encode(b) for b in blobs]
    assert [len(t) for t in ids] == counts
    eos = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id
    db = packer(S, W)
    ids_p, am, _, pos, placed = one_call(torch, db, blobs, ids, S, W, eos, f"crafted S={S} W={W}")
    db.close()
    pieces = ((pos == 0) & (am == 1)).sum(1)
    assert any(exact and not new for exact, _, _, new in placed)  # an exact fit into an open row
    assert any(moved for _, _, moved, _ in placed)                # most recent != lowest index
    assert pieces.max() >= 3 and (am == 0).any()
    if W == 8:  # a window without a kept record gives no rows; the last window is short
        assert best_fit_model.pack(ids[8:16], S, eos, W)[0].shape[0] == 0 and len(ids) % W
    if S == 4096:  # a run longer than the rows kernel stages, in a row opened with room >= 4032
        assert pieces.max() > 64


def test_two_uneven_calls(torch, native_lib, corpus):
    """The rows are those of each call on its own, not of one call; then the flush gives 0 rows."""
    S, W = 33, 7
    blobs, ids, eos = corpus
    db = packer(S, W)
    rows = []
    for a, b in [(0, 5), (5, len(ids))]:  # (the second call's windows start at record 5)
        rows.append(one_call(torch, db, blobs[a:b], ids[a:b], S, W, eos, f"records [{a}, {b})")[0])
    assert not np.array_equal(np.concatenate(rows), best_fit_model.pack(ids, S, eos, W)[0])
    assert res_rows(db.flush_device(), torch) == 0
    db.close()


def test_host_queue(native_lib, records, oracle_gpt2):
    """GenTokenizer(Gpt(pack=True, best_fit=...)), B = 4, S = 64: two bulk pushes, then
    get_working_batch until None; the batches are the two calls' rows cut into groups of 4."""
    Bsz, S, W = 4, 64, 16
    eos = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id
    ids = [oracle_gpt2.encode(t) for t in records]
    h = len(records) // 3
    calls = [best_fit_model.pack(part, S, eos, W, 64) for part in (ids[:h], ids[h:])]  # (GenTokenizer keeps the reference's min_ids)
    want = [np.concatenate([c[k] for c in calls]) for k in range(4)]
    gt = B.GenTokenizer(B.ModelType.Gpt2, B.BatchConfig(Bsz, S), B.Gpt(pack=True, best_fit=B.BestFit(W)),
                        B.TokenizerConfig(native.GPT2_PROXY_TOKENIZER), chunk=True)
    got = gt.create_sync_batches(records[:h]) + gt.create_sync_batches(records[h:])
    while (b := gt.get_working_batch()) is not None:
        got.append(b)
    gt.close()
    n = want[0].shape[0]
    assert len(got) == -(-n // Bsz) and sum(b.rows for b in got) == n
    for i, ds in enumerate(got):
        d = ds.to_dict()
        for k, name in enumerate(NAMES):
            np.testing.assert_array_equal(d[name][:ds.rows], want[k][i * Bsz:i * Bsz + ds.rows], err_msg=f"batch {i} {name}")


def test_refusals(torch, native_lib):
    L = native_lib
    fim = native.Fim(500, 500, 0, 1, 2)

    def refused(h, bf, code, word):
        assert L.sdl_batcher_set_best_fit(h, ctypes.byref(bf)) == code
        assert word in L.sdl_last_error().decode()
    ok = native.BestFit(64)
    plain = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=64, tokenizer=native.GPT2_PROXY_TOKENIZER)
    refused(plain._h, ok, -6, "pack = 1")  # SDL_ERR_STATE: not a packed clm handle
    plain.close()
    with pytest.raises(native.SDLError) as e:  # sequence_length > 4096: no such handle exists to set it on
        DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=4097, tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1)
    assert e.value.code == -1 and "sequence_length" in str(e.value)  # SDL_ERR_ARG
    db = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=64, tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1)
    for w in (0, 4097):
        refused(db._h, native.BestFit(w), -1, "window_records")
    bad = native.BestFit(64)
    bad.reserved[1] = 1
    refused(db._h, bad, -1, "reserved")
    assert L.sdl_batcher_set_best_fit(db._h, ctypes.byref(ok)) == 0  # still fresh: accepted
    assert L.sdl_batcher_set_fim(db._h, ctypes.byref(fim)) == -6 and "best fit" in L.sdl_last_error().decode()
    run(torch, db, [b"a b", b"c"])
    refused(db._h, ok, -6, "seen a record")
    db.close()
    eos = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id
    with_fim = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=64, tokenizer=native.GPT2_PROXY_TOKENIZER,
                             pack=1, fim=native.Fim(500, 500, *[i for i in range(4) if i != eos][:3]))
    refused(with_fim._h, ok, -6, "fill-in-the-middle")
    with_fim.close()
    c = native.default_config(native.SDL_TASK_CLM)  # a shard of an sdl_multi
    c.batch_size, c.sequence_length, c.pack = 4, 64, 1
    m, devs = ctypes.c_void_p(), (ctypes.c_int32 * 1)(0)
    assert L.sdl_multi_create(ctypes.byref(c), native.GPT2_PROXY_TOKENIZER.encode(), native.DATA_DIR.encode(), devs, 1,
                              ctypes.byref(m)) == 0
    refused(L.sdl_multi_handle(m, 0), ok, -4, "sdl_multi")  # SDL_ERR_UNSUPPORTED
    L.sdl_multi_destroy(m)
