"""Packed clm rows on the device (sdl_config.pack = 1, pack.hip): all four planes, exactly, against
the numpy model of the contract (tests/pack_model.py) applied to the oracle tokenizer's ids per
record -- one call at widths on and off the 4-int grid, the record filter, the carry across calls
of uneven size, the host path's batch queue, the refusals and the Transport frames."""
import ctypes
import os
import pickle
import random

import numpy as np
import pytest

import oracle_lib
import pack_model
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EOT = "<|endoftext|>"


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


def hard_blobs(seed, n):
    """Records in the style of test_gpu_gpt2.hard_blobs: every pre-tokenizer class, the literal
    end-of-text string, invalid UTF-8, pieces past 64 bytes."""
    rng = random.Random(seed)
    parts = ["a", "Z", "é", "中", "😀", " ", "  ", "\n", "\t", "'", "'s", "'ll", "'re", "1", "٣", "!", ".", EOT,
             " ", "　", "x" * 70, " " * 80, "=" * 100, "ab" * 40, "\xff", "\x80", "\xc3", "\xe2\x82"]
    out = []
    for _ in range(n):
        k = rng.choice([0, 1, 3, 10, 40, 200])
        out.append("".join(rng.choice(parts) for _ in range(k)).encode("utf-8", "surrogatepass"))
    out.append(bytes([0xC3, 0x28, 0xA0, 0xA1, 0xE2, 0x28, 0xA1, 0xF0, 0x90, 0x28, 0xBC, 0xFF, 0xFE]) * 3)
    return out


@pytest.fixture(scope="module")
def corpus(records, oracle_gpt2):
    """(blobs, ids per record, eos): the fixture records (about 100 KB: past the 64-chunk small-call
    limit) between hard records, empty records, records of exactly one id, a record with the
    literal end-of-text string mid-text and one that spans many rows at S = 33 and S = 100."""
    fixture = [t.encode("utf-8") for t in records]
    extra = hard_blobs(5, 60) + [b"", b"a", b"", b"", b"!", ("before " + EOT + " after").encode(), EOT.encode(),
                                 b"word " * 700, b"", b"z"]
    h = len(fixture) // 2
    blobs = extra[:30] + fixture[:h] + extra[30:] + fixture[h:] + [b"", b"the end"]
    assert sum(map(len, blobs)) > 65 * 1024
    ids = [oracle_gpt2.encode(b) for b in blobs]
    eos = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id
    assert eos >= 0 and oracle_gpt2.encode(EOT) == [eos]
    assert any(eos in t and len(t) > 1 for t in ids) and sum(len(t) == 1 for t in ids) >= 3
    return blobs, ids, eos


def upload(torch, blobs):
    offs = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum([len(b) for b in blobs], out=offs[1:])
    arena = np.zeros(int(offs[-1]) + 16, np.uint8)
    arena[:int(offs[-1])] = np.frombuffer(b"".join(blobs), np.uint8)
    return torch.from_numpy(arena).cuda(), torch.from_numpy(offs.astype(np.int64)).cuda(), int(offs[-1])


def run(torch, db, blobs):
    ta, to, n = upload(torch, blobs)
    res = db.process(ta.data_ptr(), n, to.data_ptr(), len(blobs))
    torch.cuda.synchronize()
    return res


def four(res, n=None):
    ids, am, tt, lab = res.planes(n)
    assert tt is None  # the public token_type_ids stays NULL for clm
    return ids, am, lab, res.position_ids(n)


def packer(S, Bsz=4, min_ids=0):
    return DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=Bsz, sequence_length=S, min_ids=min_ids,
                         tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1)


def check(got, want, what):
    for name, g, w in zip(("input_ids", "attention_mask", "labels", "position_ids"), got, want):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def check_padding(res, G, Bsz, S):
    """Rows from *d_rows to the next multiple of B: the clm padding rows' initial values."""
    n = -(-G // Bsz) * Bsz
    if n == G:
        return
    ids, am, lab, pos = four(res, n)
    assert (ids[G:] == 0).all() and (am[G:] == 1).all() and (lab[G:] == -100).all() and (pos[G:] == 0).all()


@pytest.mark.parametrize("min_ids", [0, 64])
@pytest.mark.parametrize("S", [33, 100, 128, 1024])
def test_one_call_then_flush(torch, native_lib, corpus, S, min_ids):
    blobs, ids, eos = corpus
    want = pack_model.pack(ids, S, eos, min_ids)
    db = packer(S, min_ids=min_ids)
    res = run(torch, db, blobs)
    G = want[0].shape[0]
    assert res.rows() == G and G > 4
    assert res.r.rows_capacity >= -(-G // 4) * 4 and res.r.rows_capacity % 4 == 0
    got = four(res)
    assert (got[1] == 1).all()  # every row before the flush row is full
    check(got, want[:4], f"S={S} min_ids={min_ids}")
    check_padding(res, G, 4, S)
    t = res.tensors()  # the zero-copy device views carry the fourth plane too
    assert set(t) == {"input_ids", "attention_mask", "labels", "position_ids"}
    np.testing.assert_array_equal(t["position_ids"].cpu().numpy(), want[3])
    np.testing.assert_array_equal(res.record_rows(), pack_model.record_rows(ids, min_ids))
    assert res.tokens() == sum(map(len, ids))  # d_tokens keeps its meaning: ids before framing
    if min_ids:
        assert (pack_model.record_rows(ids, min_ids) == 0).sum() > (pack_model.record_rows(ids, 0) == 0).sum()
    fl = db.flush_device()
    torch.cuda.synchronize()
    wf = pack_model.flush(want[4], S)
    assert fl.rows() == wf[0].shape[0]
    check(four(fl), wf, f"S={S} flush")
    check_padding(fl, fl.rows(), 4, S)
    again = db.flush_device()
    torch.cuda.synchronize()
    assert again.rows() == 0
    db.close()


def test_carry_across_uneven_calls(torch, native_lib, corpus):
    """S = 100: an R = 0 call, a one-record call that emits no row, a call that leaves a carry of
    exactly 0 and calls of uneven size; the rows of all calls and the flush are the one-call rows."""
    S = 100
    blobs, ids, eos = corpus
    lens = pack_model.record_rows(ids, 0).astype(np.int64)

    def choose():
        """With the model: records [a, z) whose stream ends exactly on a row end (a carry of 0),
        record a alone staying under one row."""
        for a in range(40):
            if 0 < lens[a] < S:
                ks = np.flatnonzero(np.cumsum(lens[a:]) % S == 0)
                ks = ks[(ks >= 4) & (ks < len(lens) - a - 50)]
                if ks.size:
                    return a, a + int(ks[0]) + 1
        raise AssertionError("no cut with a carry of 0 in these records")

    a0, z0 = choose()
    blobs, ids = blobs[a0:], ids[a0:]
    z, n = z0 - a0, len(blobs)
    # [0, 0): R = 0; [0, 1): no row; [1, 1): R = 0 with a carry waiting; [1, z): leaves a carry of 0
    cuts = [0, 0, 1, 1, z, z + 1, z + 40, n - 3, n]
    assert cuts == sorted(cuts)
    db = packer(S)
    carry = pack_model.EMPTY
    rows = [[], [], [], []]
    saw = set()
    for a, b in zip(cuts[:-1], cuts[1:]):
        want = pack_model.pack(ids[a:b], S, eos, 0, carry)
        res = run(torch, db, blobs[a:b])
        G = want[0].shape[0]
        assert res.rows() == G, (a, b)
        got = four(res)
        check(got, want[:4], f"records [{a}, {b})")
        check_padding(res, G, 4, S)
        carry = want[4]
        for k in range(4):
            rows[k].append(got[k])
        saw |= {"R0" if a == b else "", "norow" if b > a and G == 0 else "", "carry0" if b > a and len(carry[0]) == 0 else ""}
    assert {"R0", "norow", "carry0"} <= saw
    fl = db.flush_device()
    torch.cuda.synchronize()
    gf = four(fl)
    assert db.flush_device().rows() == 0  # a second flush emits nothing
    one = pack_model.pack(ids, S, eos, 0)
    wf = pack_model.flush(one[4], S)
    for k in range(4):
        np.testing.assert_array_equal(np.concatenate(rows[k] + [gf[k]]), np.concatenate([one[k], wf[k]]))
    db.close()


def test_host_path_batches(native_lib, records, oracle_gpt2):
    """GenTokenizer(Gpt(pack=True)), B = 4, S = 64: per-record pushes, then get_working_batch until
    None; the batches are the model's rows (flush row included) cut into groups of 4."""
    Bsz, S = 4, 64
    eos = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).eos_id
    ids = [oracle_gpt2.encode(t) for t in records]
    one = pack_model.pack(ids, S, eos, 64)  # (GenTokenizer keeps the reference's min_ids)
    wf = pack_model.flush(one[4], S)
    want = [np.concatenate([one[k], wf[k]]) for k in range(4)]
    n = want[0].shape[0]
    gt = B.GenTokenizer(B.ModelType.Gpt2, B.BatchConfig(Bsz, S), B.Gpt(pack=True),
                        B.TokenizerConfig(native.GPT2_PROXY_TOKENIZER), chunk=True)
    got = [b for b in (gt.create_sync_batch(t) for t in records) if b is not None]
    assert all(b.rows == Bsz for b in got)
    while True:
        b = gt.get_working_batch()
        if b is None:
            break
        got.append(b)
    assert gt.get_working_batch() is None
    assert len(got) == -(-n // Bsz) and sum(b.rows for b in got) == n
    for i, ds in enumerate(got):
        assert ds.token_type_ids is None and ds.rows == min(Bsz, n - i * Bsz)
        d = ds.to_dict()
        assert set(d) == {"input_ids", "attention_mask", "labels", "position_ids"}
        sl = slice(i * Bsz, i * Bsz + ds.rows)
        for k, name in enumerate(("input_ids", "attention_mask", "labels", "position_ids")):
            np.testing.assert_array_equal(d[name][:ds.rows], want[k][sl], err_msg=f"batch {i} {name}")
        # rows of the last batch nobody filled: the initial values
        assert (ds.input_ids[ds.rows:] == 0).all() and (ds.attention_mask[ds.rows:] == 1).all()
        assert (ds.labels[ds.rows:] == -100).all() and (ds.position_ids[ds.rows:] == 0).all()
    gt.close()
    # the same records in one bulk call queue the same batches
    gt = B.GenTokenizer(B.ModelType.Gpt2, B.BatchConfig(Bsz, S), B.Gpt(pack=True),
                        B.TokenizerConfig(native.GPT2_PROXY_TOKENIZER), chunk=True)
    bulk = gt.create_sync_batches(records)
    assert len(bulk) == n // Bsz or len(bulk) == (n - 1) // Bsz  # (the flush row is not there yet)
    for i, ds in enumerate(bulk):
        np.testing.assert_array_equal(ds.input_ids, got[i].input_ids)
        np.testing.assert_array_equal(ds.position_ids, got[i].position_ids)
    gt.close()


def test_default_did_not_move(native_lib, records):
    """pack=False at the golden's shape: test_gpu_gpt2.test_clm_stream_matches_golden's check."""
    g = np.load(os.path.join(GOLDEN, "clm_s128_b8.npz"))
    gt = B.GenTokenizer(B.ModelType.Gpt2, B.BatchConfig(8, 128), B.Gpt(pack=False),
                        B.TokenizerConfig(native.GPT2_PROXY_TOKENIZER), chunk=True)
    got = [b for b in (gt.create_sync_batch(t) for t in records) if b is not None]
    got.append(gt.get_working_batch())
    assert len(got) == int(g["n_batches"])
    for i, ds in enumerate(got):
        assert ds.rows == int(g[f"b{i}_rows"])
        assert ds.token_type_ids is None and ds.position_ids is None
        np.testing.assert_array_equal(ds.input_ids, g[f"b{i}_input_ids"])
        np.testing.assert_array_equal(ds.attention_mask, g[f"b{i}_attention_mask"])
        np.testing.assert_array_equal(ds.labels, g[f"b{i}_labels"])
        assert set(ds.to_dict()) == {"input_ids", "attention_mask", "labels"}
    gt.close()
    # ... and an unpacked handle has no position plane and no flush row
    db = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=64, tokenizer=native.GPT2_PROXY_TOKENIZER)
    assert not native_lib.sdl_device_position_ids(db._h)
    out = native.DeviceRows()
    assert native_lib.sdl_pack_flush_device(db._h, None, ctypes.byref(out)) == -6  # SDL_ERR_STATE
    db.close()


@pytest.mark.parametrize("tok", [native.BERT_PROXY_TOKENIZER, native.T5_PROXY_TOKENIZER], ids=["bert", "t5"])
def test_other_tokenizers_are_refused(native_lib, tok):
    c = native.default_config(native.SDL_TASK_CLM)
    c.pack = 1
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), tok.encode(), native.DATA_DIR.encode(), ctypes.byref(h))
    assert rc == -4 and not h.value  # SDL_ERR_UNSUPPORTED
    msg = native_lib.sdl_last_error().decode()
    assert "pack" in msg and "byte-level BPE" in msg


def test_json_to_frames_is_refused(native_lib):
    db = packer(64)
    with pytest.raises(native.SDLError) as e:
        db.json_to_frames(b'{"text": "a b c"}\n')
    assert e.value.code == -4 and "pack" in str(e.value)
    db.close()


def test_frames_of_a_packed_call(torch, native_lib, corpus):
    """sdl_pickle_frames_device over a packed call's rows: the reference's three keys, packed planes."""
    Bsz, S = 4, 100
    blobs, ids, eos = corpus
    want = pack_model.pack(ids, S, eos, 0)
    db = packer(S, Bsz)
    res = run(torch, db, blobs)
    n = res.rows()
    assert n == want[0].shape[0] and n > Bsz
    fr = db.pickle_frames(res, n, flush_partial=True)
    torch.cuda.synchronize()
    nb = -(-n // Bsz)
    assert len(fr) == nb
    frames = fr.frames()
    p_ids, p_am, _, p_lab = res.planes(nb * Bsz)
    for b, frame in enumerate(frames):
        rows = min(Bsz, n - b * Bsz)
        sl = slice(b * Bsz, (b + 1) * Bsz)
        assert frame == oracle_lib.pickle_dataset("clm", Bsz, S, S, rows, p_ids[sl], p_am[sl], None, p_lab[sl]), b
    d = pickle.loads(frames[0])
    assert list(d) == ["input_ids", "attention_mask", "labels"]
    assert d["input_ids"] == want[0][:Bsz].tolist() and d["labels"] == want[2][:Bsz].tolist()
    assert d["attention_mask"] == want[1][:Bsz].tolist()
    db.close()
