"""Packed mlm rows over a byte-level BPE tokenizer in RoBERTa's form (pack_mlm_bpe.hip): all five
planes, exactly, against the model of the contract (tests/pack_mlm_bpe_model.py) over the gpt2
oracle's ids -- one call and the flush row, calls of uneven size, the host path, the refusals.  The
corpus holds every way the row's segment table can go wrong; each is asserted on the model's planes."""
import ctypes

import numpy as np
import pytest

import mlm_policy_model as M
import pack_mlm_bpe_model as model
import pack_mlm_model
import pack_model
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher
from test_gpu_pack_mlm import check, check_padding, five, run, torch  # noqa: F401  (torch: the fixture)

pytestmark = pytest.mark.gpu
SEED, BSZ = 77, 4


@pytest.fixture(scope="module")
def tk(tmp_path_factory):
    return model.roberta_tokenizer(tmp_path_factory.mktemp("roberta") / "tokenizer.json")


@pytest.fixture(scope="module")
def corpus(oracle_gpt2):
    """(texts, ids per record): 110 one-word documents, then three empty records, documents of 9 to 78
    words each behind a run of empty records, documents dense with "!" (id 0), one holding the literal
    </s>, one of 1100 words, and a short tail."""
    words = [M.COMMON[(7 * i) % len(M.COMMON)] for i in range(1100)]
    texts = words[:110] + ["", "", ""]
    for i in range(24):
        texts += [""] * (1 + i % 3) + [" ".join(words[i:i + 9 + 3 * i])]
    texts += [" ".join(w + "!" for w in words[i:i + 30]) for i in range(6)]
    texts += ["one two three </s> four five six seven eight", " ".join(words), "", "to be"]
    ids = [sum((oracle_gpt2.encode(part) + [model.SEP] for part in t.split("</s>")), [])[:-1] for t in texts]
    return texts, ids


def packer(tk, S, policy, min_ids=0):
    return DeviceBatcher(batch_size=BSZ, sequence_length=S, seed=SEED, min_ids=min_ids, mask_policy=policy, pack=1,
                         tokenizer=tk.path, mask_id=tk.mask)


def mask_length(S):
    return int(np.float32(S) * np.float32(0.15))


@pytest.mark.parametrize("min_ids", [0, 8])
@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("S", [30, 64, 300])
def test_one_call_then_flush(torch, native_lib, tk, corpus, S, policy, min_ids):
    texts, ids = corpus
    want, carry = model.pack(ids, S, min_ids, pack_model.EMPTY, 0, tk, policy, SEED, mask_length(S))
    rr = pack_mlm_model.record_rows(ids, min_ids)  # n + 2, or 0
    G = want.shape[1]
    # the corpus' conditions, on the model: the unmasked ids, every kept record's stream offset
    orig, pos = np.where(want[3] != -100, want[3], want[0]), want[4]
    off = np.cumsum(rr) - rr
    starts = [(pos[g] == 0).sum() for g in range(G)]
    if min_ids == 0 and S == 300:  # more than 64 segments in a row: a second batch of boundaries
        assert max(starts) > 64
    first_in_row = [r for r in range(1, len(rr)) if rr[r] and off[r] < G * S and
                    not any(rr[s] and off[s] // S == off[r] // S for s in range(r))]
    assert any(rr[r - 1] == 0 for r in first_in_row)  # dropped records right before a row's first document
    assert ((rr[:-1] == 0) & (rr[1:] == 0)).sum() >= (100 if min_ids else 10)  # ... and in runs
    assert any((pos[g] == np.arange(S)).all() and orig[g, 0] != tk.cls for g in range(G))  # no start bit in the row
    assert (want[3] == 0).any()  # a picked "!": id 0 is a candidate
    assert tk.sep in ids[-4] and rr[-4]  # the literal </s> inside a kept document
    db = packer(tk, S, policy, min_ids)
    res = run(torch, db, texts)
    assert res.rows() == G and G > BSZ
    check(five(res), want, f"S={S} policy={policy} min_ids={min_ids}")
    check_padding(res, G)
    np.testing.assert_array_equal(res.record_rows(), rr)
    fl = db.flush_device()
    torch.cuda.synchronize()
    wf = model.flush(carry, S, G, tk, policy, SEED, mask_length(S))
    c = len(carry[0])
    assert fl.rows() == wf.shape[1] == 1 and 0 < c < S
    assert (wf[:, 0, c:] == np.array([tk.pad, 0, 0, -100, 0])[:, None]).all()  # <pad> / 0 / (0) / -100 / 0
    check(five(fl), wf, f"S={S} flush")
    check_padding(fl, 1)
    assert db.flush_device().rows() == 0
    db.close()


@pytest.mark.parametrize("S,policy", [(1024, 2), (2048, 1), (2048, 2)])
def test_wide_rows(torch, native_lib, tk, corpus, S, policy):
    """Four and eight rounds a lane (the kernels' other instantiations, the widest LDS layout): four
    passes over the corpus in one call, then the flush row."""
    texts, ids = corpus[0] * 4, corpus[1] * 4
    want, carry = model.pack(ids, S, 0, pack_model.EMPTY, 0, tk, policy, SEED, mask_length(S))
    assert want.shape[1] >= 5 and max((want[4][g] == 0).sum() for g in range(want.shape[1])) > 128
    db = packer(tk, S, policy)
    res = run(torch, db, texts)
    check(five(res), want, f"S={S} policy={policy}")
    fl = db.flush_device()
    torch.cuda.synchronize()
    check(five(fl), model.flush(carry, S, want.shape[1], tk, policy, SEED, mask_length(S)), f"S={S} flush")
    db.close()


@pytest.mark.parametrize("S,policy", [(64, 2), (30, 1)])
def test_uneven_calls_equal_one_call(torch, native_lib, tk, corpus, S, policy):
    """A call of one record, a call of only dropped records (the three empty ones), calls of uneven
    size: row for row the rows of one call over all records, flush row included."""
    texts, ids = corpus
    n = len(texts)
    cuts = [0, 1, 50, 110, 113, 120, n - 2, n]
    assert not any(ids[110:113])
    db = packer(tk, S, policy)
    rows = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        res = run(torch, db, texts[a:b])
        rows.append(five(res, res.rows()))
        check_padding(res, res.rows())
    fl = db.flush_device()
    torch.cuda.synchronize()
    rows.append(five(fl))
    want, carry = model.pack(ids, S, 0, pack_model.EMPTY, 0, tk, policy, SEED, mask_length(S))
    wf = model.flush(carry, S, want.shape[1], tk, policy, SEED, mask_length(S))
    check(np.concatenate(rows, axis=1), np.concatenate([want, wf], axis=1), f"S={S} calls {cuts}")
    db.close()


def test_host_path_batches(native_lib, tk, corpus):
    """GenTokenizer(ModelType.Roberta, Mask(pack=True)), B = 4, S = 64: per-record pushes, then
    get_working_batch until None; the batches are the model's rows (flush row included) in groups of 4."""
    S, ml = 64, 9
    texts, ids = corpus
    one, carry = model.pack(ids, S, 64, pack_model.EMPTY, 0, tk, 1, SEED, ml)  # (GenTokenizer keeps the reference's min_ids)
    want = np.concatenate([one, model.flush(carry, S, one.shape[1], tk, 1, SEED, ml)], axis=1)
    n = want.shape[1]
    gt = B.GenTokenizer(B.ModelType.Roberta, B.BatchConfig(BSZ, S), B.Mask(ml, tk.mask, mask_policy=1, pack=True),
                        B.TokenizerConfig(tk.path), chunk=True, seed=SEED)
    got = [b for b in (gt.create_sync_batch(t) for t in texts) if b is not None]
    while True:
        b = gt.get_working_batch()
        if b is None:
            break
        got.append(b)
    assert len(got) == -(-n // BSZ) and sum(b.rows for b in got) == n > BSZ
    for i, ds in enumerate(got):
        d = ds.to_dict()
        for k, name in enumerate(("input_ids", "attention_mask", "token_type_ids", "labels", "position_ids")):
            np.testing.assert_array_equal(d[name][:ds.rows], want[k][i * BSZ:i * BSZ + ds.rows], err_msg=f"batch {i} {name}")
    gt.close()


def test_refusals(native_lib, tk, tmp_path):
    def create(path, **kw):
        c = native.default_config(native.SDL_TASK_MLM)
        c.pack, c.mask_policy, c.mask_id = 1, 1, tk.mask
        for k, v in kw.items():
            setattr(c, k, v)
        h = ctypes.c_void_p()
        rc = native_lib.sdl_batcher_create(ctypes.byref(c), path.encode(), native.DATA_DIR.encode(), ctypes.byref(h))
        assert not h.value
        return rc, native_lib.sdl_last_error().decode()
    rc, msg = create(native.GPT2_PROXY_TOKENIZER)
    assert rc == -4 and "pack" in msg and "WordPiece" in msg and "RobertaProcessing" in msg
    rc, msg = create(model.roberta_tokenizer(tmp_path / "tokenizer.json", pad=False).path)
    assert rc == -4 and "<pad>" in msg
    rc, msg = create(tk.path, pack=0, mask_policy=2)
    assert rc == -4 and "mask_policy 2" in msg
    db = packer(tk, 64, 1)
    with pytest.raises(native.SDLError) as e:
        db.json_to_frames(b'{"text": "a b c"}\n')
    assert e.value.code == -4 and "pack" in str(e.value)
    db.close()
