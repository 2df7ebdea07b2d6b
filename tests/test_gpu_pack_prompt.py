"""Prompt / completion examples in packed clm rows (sdl_config.pair = 6, pack_prompt.hip): all four
planes, exactly, against a plain model of the contract (include/sdl_batcher.h "Prompt / completion
examples"; tests/pack_prompt_model.py over tests/pack_model.py) on the oracle tokenizer's ids per
text range."""
import ctypes

import numpy as np
import pytest

import pack_prompt_model as model
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher
from test_gpu_pack import check, four, packer, upload

pytestmark = pytest.mark.gpu
NAMES = ("input_ids", "attention_mask", "labels", "position_ids")
PAIR = native.SDL_PAIR_CLM_COMPLETION


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def corpus(records, oracle_gpt2):
    """(pairs of blobs, pairs of id lists, eos): a prompt of 64 k ids first (its seam is a row start
    at S = 64), the hand-made pairs, the fixture records two by two, and a prompt of more than
    3 * 64 ids with a short completion."""
    fixture = [t.encode("utf-8") for t in records]
    long_a = b" ".join(fixture[:12])
    pairs = [(b" a" * 64, b" b"), (b"", b"a"), (b"a", b""), (b"", b""), (b"a", b" b")] + \
        list(zip(fixture[0::2], fixture[1::2])) + [(long_a, b" yes")]
    ids = [(oracle_gpt2.encode(a), oracle_gpt2.encode(b)) for a, b in pairs]
    assert len(ids[0][0]) % 64 == 0 and len(ids[-1][0]) > 3 * 64 and [len(x) for x in ids[4]] == [1, 1]
    return pairs, ids, native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id


def prompt_packer(S, min_ids=0):
    return DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=S, min_ids=min_ids,
                         tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1, pair=PAIR)


def run_pairs(torch, db, pairs):
    ta, to, n = upload(torch, [t for p in pairs for t in p])
    res = db.process_pairs(ta.data_ptr(), n, to.data_ptr(), len(pairs))
    torch.cuda.synchronize()
    return res


def rows_of(torch, db, calls):
    """The rows of the calls and the flush, concatenated per plane, and the calls' d_record_rows."""
    got, rec = [[] for _ in NAMES], []
    for pairs in calls:
        res = run_pairs(torch, db, pairs)
        rec.append(res.record_rows())
        for k, plane in enumerate(four(res)):
            got[k].append(plane)
    fl = db.flush_device()
    torch.cuda.synchronize()
    for k, plane in enumerate(four(fl)):
        got[k].append(plane)
    return [np.concatenate(g) for g in got], np.concatenate(rec)


def with_flush(want, S):
    return [np.concatenate([want[k], f]) for k, f in enumerate(model.flush(want[4], S))]


def layout(ids, min_ids=0):
    """Per example (stream start, nA, length): the model's stream positions from an empty carry."""
    n = model.record_rows(ids, min_ids).astype(np.int64)
    return list(zip(np.cumsum(n) - n, [len(a) for a, _ in ids], n))


@pytest.mark.parametrize("S", [30, 33, 64])  # off the 4-int grid, odd, aligned
def test_one_call_then_flush(torch, native_lib, corpus, S):
    pairs, ids, eos = corpus
    want = model.pack(ids, S, eos)
    # conditions on the inputs, shown by the model
    lay = layout(ids)
    doc = [(s, nA, n) for s, nA, n in lay if n]
    seams = [s + nA for s, nA, n in doc if nA]
    assert any(n == 0 for _, _, n in lay) and any(nA == 0 for _, nA, _ in doc)  # a dropped pair, a kept empty prompt
    assert (want[2] == -100).all(axis=1).any()  # a row wholly inside a prompt
    assert any(p % 4 for p in seams) and any(p % 4 == 0 for p in seams)  # a seam inside a 4-position group, one at its start
    assert any((s + n) % 4 for s, _, n in doc)  # a document end inside a group (a row end is, whenever S % 4 != 0)
    assert S != 64 or any(p % S == 0 for p in seams)  # a seam exactly at a row start
    db = prompt_packer(S)
    got, rec = rows_of(torch, db, [pairs])
    db.close()
    check(got, with_flush(want, S), f"S={S}")
    np.testing.assert_array_equal(rec, model.record_rows(ids))


def test_split_invariance(torch, native_lib, corpus):
    """Three uneven calls and a flush give the rows of one call and a flush.  A call is made of whole
    examples, so its stream ends behind an eos; what can fall inside an example is the end of the
    call's last full row.  The first call's falls strictly inside a prompt (the carry opens with
    prompt flags, and the completion behind them carries labels), the second call's strictly inside
    the completion of an example with a prompt (that prompt left in the rows, the carry opens with
    label positions)."""
    S = 33
    pairs, ids, eos = corpus
    lay = layout(ids)

    def row_end_in(k, lo, hi):  # examples [0, k): the last full row of their stream ends in [start + lo, start + hi) of one
        cut = (lay[k - 1][0] + lay[k - 1][2]) // S * S
        return any(n and nA and s + lo(nA) < cut < s + hi(nA, n) for s, nA, n in lay[:k])
    k1 = next(k for k in range(8, len(ids)) if row_end_in(k, lambda nA: 0, lambda nA, n: nA))
    k2 = next(k for k in range(k1 + 5, len(ids)) if row_end_in(k, lambda nA: nA, lambda nA, n: n - 1))
    cuts = [0, k1, k2, len(ids)]
    want = model.pack(ids, S, eos)
    db = prompt_packer(S)
    got, rec = rows_of(torch, db, [pairs[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    db.close()
    check(got, with_flush(want, S), "three calls")
    np.testing.assert_array_equal(rec, model.record_rows(ids))


def test_min_ids(torch, native_lib, oracle_gpt2):
    """min_ids = 8 drops the example of 7 positions and keeps the one of 8; two calls short of a row
    first, so the carry (flags included) is also copied in front of a call that emits no row."""
    S, min_ids = 33, 8
    pairs = [(b"a b c", b" d e f g"), (b"a b c", b" d e f"), (b"", b" d e f g h i j"), (b"a b c d e f g h", b""),
             (b"a b", b" c d e f g h i j k l m n o p q r s t u v w x y z")]
    ids = [(oracle_gpt2.encode(a), oracle_gpt2.encode(b)) for a, b in pairs]
    eos = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id
    assert [len(a) + len(b) + 1 for a, b in ids[:2]] == [8, 7]
    np.testing.assert_array_equal(model.record_rows(ids, min_ids)[:4] > 0, [True, False, True, False])
    assert model.record_rows(ids, min_ids)[:3].sum() < S < model.record_rows(ids, min_ids).sum()
    want = model.pack(ids, S, eos, min_ids)
    db = prompt_packer(S, min_ids)
    got, rec = rows_of(torch, db, [pairs[:1], pairs[1:3], pairs[3:]])
    db.close()
    check(got, with_flush(want, S), "min_ids")
    np.testing.assert_array_equal(rec, model.record_rows(ids, min_ids))


def test_host_path_batches(native_lib, records, oracle_gpt2):
    """GenTokenizer(Gpt(pack=True, completion_only=True)), B = 4, S = 64: two bulk pushes, then
    get_working_batch until None; the batches are the model's rows (flush row included) in groups of 4."""
    Bsz, S = 4, 64
    pairs = list(zip(records[0::2], records[1::2]))
    ids = [(oracle_gpt2.encode(a), oracle_gpt2.encode(b)) for a, b in pairs]
    eos = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id
    want = with_flush(model.pack(ids, S, eos, 64), S)  # (GenTokenizer keeps the reference's min_ids)
    gt = B.GenTokenizer(B.ModelType.Gpt2, B.BatchConfig(Bsz, S), B.Gpt(pack=True, completion_only=True),
                        B.TokenizerConfig(native.GPT2_PROXY_TOKENIZER), chunk=True)
    h = len(pairs) // 3
    got = gt.create_sync_batches_pairs(pairs[:h]) + gt.create_sync_batches_pairs(pairs[h:])
    while (b := gt.get_working_batch()) is not None:
        got.append(b)
    gt.close()
    n = want[0].shape[0]
    assert len(got) == -(-n // Bsz) and sum(b.rows for b in got) == n
    for i, ds in enumerate(got):
        d = ds.to_dict()
        for k, name in enumerate(NAMES):
            np.testing.assert_array_equal(d[name][:ds.rows], want[k][i * Bsz:i * Bsz + ds.rows], err_msg=f"batch {i} {name}")


def _push(L, h, pair):
    one, off = ctypes.create_string_buffer(b"a b"), (ctypes.c_uint64 * 3)(0, 1, 3)
    if pair:
        return [L.sdl_batcher_push_pair(h, one, 1, one, 2, None, 0, None),
                L.sdl_batcher_push_many_pairs(h, one, off, 1, None, None, None)]
    return [L.sdl_batcher_push(h, one, 3, None, 0, None), L.sdl_batcher_push_many(h, one, off, 2, None, None, None)]


@pytest.mark.parametrize("case", ["unpaired calls", "pair calls on plain pack", "set_fim", "set_best_fit", "json_to_frames",
                                  "multi_create", native.BERT_PROXY_TOKENIZER, native.T5_PROXY_TOKENIZER])
def test_refusals(torch, native_lib, case):
    """The refusals that need a device (tests/test_pack_prompt_config.py has the config's own): code and named word."""
    L = native_lib
    if case.endswith(".json"):  # a WordPiece / Unigram tokenizer: pair = 1's code for the wrong tokenizer
        with pytest.raises(native.SDLError) as e:
            DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=64, tokenizer=case, pack=1, pair=PAIR)
        assert e.value.code == -4 and "pair" in str(e.value)
        return
    db = packer(64) if case == "pair calls on plain pack" else prompt_packer(64)
    ta, to, n = upload(torch, [b"a", b" b"])
    out = native.DeviceRows()
    dev = (ctypes.c_void_p(ta.data_ptr()), n, ctypes.c_void_p(to.data_ptr()))
    if case == "unpaired calls":
        rcs, code = _push(L, db._h, False) + [L.sdl_process_device(db._h, *dev, 2, 0, None, ctypes.byref(out))], -6
    elif case == "pair calls on plain pack":
        rcs, code = _push(L, db._h, True) + [L.sdl_process_device_pairs(db._h, *dev, 1, None, None, 0, None, ctypes.byref(out))], -6
    elif case == "set_fim":
        rcs, code = [L.sdl_batcher_set_fim(db._h, ctypes.byref(native.Fim(500, 500, 1, 2, 3)))], -6
    elif case == "set_best_fit":
        rcs, code = [L.sdl_batcher_set_best_fit(db._h, ctypes.byref(native.BestFit(64)))], -6
    elif case == "json_to_frames":
        st = native.JsonFramesStats()
        rcs, code = [L.sdl_json_to_frames(db._h, None, 0, 0, 1, ctypes.cast(None, native.FRAME_SINK), None, ctypes.byref(st))], -4
    else:
        m, dv = ctypes.c_void_p(), (ctypes.c_int32 * 1)(0)
        rcs, code = [L.sdl_multi_create(ctypes.byref(db.cfg), native.GPT2_PROXY_TOKENIZER.encode(), native.DATA_DIR.encode(),
                                        dv, 1, ctypes.byref(m))], -4
    for rc in rcs:  # (each call leaves its own message: the last one is checked below, the codes all)
        assert rc == code
    assert b"pair" in L.sdl_last_error()
    db.close()
