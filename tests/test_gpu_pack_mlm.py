"""Packed mlm rows on the device (sdl_config.pack = 1 under the MLM task, pack_mlm.hip): all five
planes, exactly, against the model of the contract (tests/pack_mlm_model.py) over the oracle
tokenizer's ids of mlm_policy_model.synthetic_texts() -- one call and the flush row at widths on
and off the 4-int grid, calls of uneven size, the host path's batch queue, the frames, the refusals."""
import ctypes
import pickle

import numpy as np
import pytest

import mlm_policy_model as M
import oracle_lib
import pack_mlm_model as model
import pack_model
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher

pytestmark = pytest.mark.gpu
SEED, BSZ = 77, 4
NAMES = ("input_ids", "attention_mask", "token_type_ids", "labels", "position_ids")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def corpus(oracle_tok):
    """(texts, ids per record): a one-word record first, the synthetic records, and between them
    runs of empty and short records -- 120 documents of 1 to 7 words, many to a row (under
    min_ids = 64 a run of dropped records, which share a stream offset)."""
    syn = M.synthetic_texts()
    shorts = [" ".join(M.COMMON[i % 50:i % 50 + 1 + i % 7]) for i in range(120)]
    texts = ["the"] + syn[:10] + ["", "the of and", "a", ""] + shorts + syn[10:] + ["", "to be"]
    return texts, [oracle_tok.encode(t)[1:-1] for t in texts]  # (encode gives [CLS] ids [SEP])


def packer(S, policy, min_ids=0):
    return DeviceBatcher(batch_size=BSZ, sequence_length=S, seed=SEED, min_ids=min_ids, mask_policy=policy, pack=1)


def run(torch, db, texts):
    blobs = [t.encode("utf-8") for t in texts]
    offs = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=offs[1:])
    arena = np.zeros(int(offs[-1]) + 16, np.uint8)
    arena[:int(offs[-1])] = np.frombuffer(b"".join(blobs), np.uint8)
    ta, to = torch.from_numpy(arena).cuda(), torch.from_numpy(offs).cuda()
    res = db.process(ta.data_ptr(), int(offs[-1]), to.data_ptr(), len(blobs))
    torch.cuda.synchronize()
    return res


def five(res, n=None):
    ids, am, tt, lab = res.planes(n)
    assert tt is not None  # token_type_ids stays non-NULL, as for unpacked mlm
    return np.stack([ids, am, tt, lab, res.position_ids(n)])


def check(got, want, what):
    for k, name in enumerate(NAMES):
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {name}")


def check_padding(res, G):
    n = -(-G // BSZ) * BSZ
    if n > G:
        p = five(res, n)[:, G:]
        assert (p[0] == 0).all() and (p[1] == 1).all() and (p[2] == 0).all() and (p[3] == -100).all() and (p[4] == 0).all()


@pytest.mark.parametrize("min_ids", [0, 64])
@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("S", [33, 128, 300, 1024])
def test_one_call_then_flush(torch, native_lib, corpus, S, policy, min_ids):
    texts, ids = corpus
    ml = int(np.float32(S) * np.float32(0.15))
    want, carry = model.pack(ids, S, min_ids, pack_model.EMPTY, 0, policy, SEED, ml)
    rr = model.record_rows(ids, min_ids)
    if min_ids:  # a run of adjacent dropped records
        assert ((rr[:-1] == 0) & (rr[1:] == 0)).sum() >= 2
    db = packer(S, policy, min_ids)
    res = run(torch, db, texts)
    G = want.shape[1]
    assert res.rows() == G and G > BSZ
    assert res.r.rows_capacity >= -(-G // BSZ) * BSZ and res.r.rows_capacity % BSZ == 0
    got = five(res)
    assert (want[3] != -100).any()  # (the model masks something)
    check(got, want, f"S={S} policy={policy} min_ids={min_ids}")
    check_padding(res, G)
    np.testing.assert_array_equal(res.record_rows(), rr)
    assert res.tokens() == sum(map(len, ids))  # d_tokens keeps its meaning: ids before framing
    fl = db.flush_device()
    torch.cuda.synchronize()
    wf = model.flush(carry, S, G, policy, SEED, ml)
    assert fl.rows() == wf.shape[1]
    check(five(fl), wf, f"S={S} flush")
    check_padding(fl, fl.rows())
    assert db.flush_device().rows() == 0
    db.close()


@pytest.mark.parametrize("S,policy", [(128, 2), (33, 1)])
def test_uneven_calls_equal_one_call(torch, native_lib, corpus, S, policy):
    """An R = 0 call, a one-record call that emits no row, an R = 0 call with a carry waiting, then
    calls of uneven size: row for row the rows of one call over all records, flush row included."""
    texts, ids = corpus
    ml = int(np.float32(S) * np.float32(0.15))
    n = len(texts)
    cuts = [0, 0, 1, 1, 7, 13, 14, n - 3, n]
    db = packer(S, policy)
    rows = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        res = run(torch, db, texts[a:b])
        G = res.rows()
        assert (a, b) != (0, 1) or G == 0
        rows.append(five(res, G))
        check_padding(res, G)
    fl = db.flush_device()
    torch.cuda.synchronize()
    rows.append(five(fl))
    want, carry = model.pack(ids, S, 0, pack_model.EMPTY, 0, policy, SEED, ml)
    wf = model.flush(carry, S, want.shape[1], policy, SEED, ml)
    assert wf.shape[1] == 1
    check(np.concatenate(rows, axis=1), np.concatenate([want, wf], axis=1), f"S={S} calls {cuts}")
    db.close()


def test_host_path_batches(native_lib, corpus):
    """GenTokenizer(Mask(pack=True)), B = 4, S = 64: per-record pushes, then get_working_batch until
    None; the batches are the model's rows (flush row included) cut into groups of 4."""
    S, ml = 64, 9
    texts, ids = corpus
    one, carry = model.pack(ids, S, 64, pack_model.EMPTY, 0, 1, SEED, ml)  # (GenTokenizer keeps the reference's min_ids)
    want = np.concatenate([one, model.flush(carry, S, one.shape[1], 1, SEED, ml)], axis=1)
    n = want.shape[1]
    gt = B.GenTokenizer(B.ModelType.Bert, B.BatchConfig(BSZ, S), B.Mask(ml, 103, mask_policy=1, pack=True),
                        B.TokenizerConfig(), chunk=True, seed=SEED)
    got = [b for b in (gt.create_sync_batch(t) for t in texts) if b is not None]
    while True:
        b = gt.get_working_batch()
        if b is None:
            break
        got.append(b)
    assert len(got) == -(-n // BSZ) and sum(b.rows for b in got) == n
    for i, ds in enumerate(got):
        d = ds.to_dict()
        assert set(d) == {"input_ids", "attention_mask", "token_type_ids", "labels", "position_ids"}
        assert (ds.token_type_ids == 0).all()
        for k, name in enumerate(NAMES):
            np.testing.assert_array_equal(d[name][:ds.rows], want[k][i * BSZ:i * BSZ + ds.rows], err_msg=f"batch {i} {name}")
    gt.close()


def test_frames_of_a_packed_call(torch, native_lib, corpus):
    """sdl_pickle_frames_device over a packed call's rows: the four mlm keys, packed planes."""
    S = 128
    texts, ids = corpus
    want, _ = model.pack(ids, S, 0, pack_model.EMPTY, 0, 1, SEED, 19)
    db = packer(S, 1)
    res = run(torch, db, texts)
    n = res.rows()
    assert n == want.shape[1] and n > BSZ
    fr = db.pickle_frames(res, n, flush_partial=True)
    torch.cuda.synchronize()
    frames = fr.frames()
    assert len(frames) == -(-n // BSZ)
    p = five(res, len(frames) * BSZ)
    for b, frame in enumerate(frames):
        sl = slice(b * BSZ, (b + 1) * BSZ)
        assert frame == oracle_lib.pickle_dataset("mlm", BSZ, S, S, min(BSZ, n - b * BSZ), p[0][sl], p[1][sl], p[2][sl],
                                                  p[3][sl]), b
    d = pickle.loads(frames[0])
    assert list(d) == ["input_ids", "attention_mask", "token_type_ids", "labels"]
    assert d["input_ids"] == want[0][:BSZ].tolist() and d["labels"] == want[3][:BSZ].tolist()
    db.close()


def test_refusals(native_lib):
    c = native.default_config(native.SDL_TASK_MLM)
    c.pack, c.mask_policy = 1, 1
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), native.GPT2_PROXY_TOKENIZER.encode(), native.DATA_DIR.encode(),
                                       ctypes.byref(h))
    assert rc == -4 and not h.value  # SDL_ERR_UNSUPPORTED
    msg = native_lib.sdl_last_error().decode()
    assert "pack" in msg and "WordPiece" in msg
    db = packer(64, 1)
    with pytest.raises(native.SDLError) as e:
        db.json_to_frames(b'{"text": "a b c"}\n')
    assert e.value.code == -4 and "pack" in str(e.value)
    db.close()
