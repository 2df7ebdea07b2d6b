"""Fill-in-the-middle documents in packed clm rows (sdl_batcher_set_fim, pack_fim.hip): all four planes,
exactly, against a plain model of the contract (include/sdl_batcher.h "Fill-in-the-middle") -- the
Philox draw of tests/mlm_policy_model.py, list slicing for the permutation, tests/pack_model.py for
the rows -- over the oracle tokenizer's ids per record."""
import ctypes

import numpy as np
import pytest

import pack_model
from mlm_policy_model import M32, philox4x32_10
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher
from test_gpu_pack import check, four, run

pytestmark = pytest.mark.gpu
SEED = 1  # (the conditions test_one_call_then_flush and test_split_invariance assert on the model hold for it)
NAMES = ("input_ids", "attention_mask", "labels", "position_ids")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def corpus(records, oracle_gpt2):
    """(blobs, ids per record, eos, the three sentinel ids): the fixture records between hand-made
    ones of 1, 2 and 3 ids and empty ones."""
    small = [b"a", b"a b", b"a b c", b""]
    blobs = small + [t.encode("utf-8") for t in records] + small[::-1]
    ids = [oracle_gpt2.encode(b) for b in blobs]
    assert [len(t) for t in ids[:4]] == [1, 2, 3, 0]
    info = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER)
    sent = [i for i in range(info.vocab_size - 1, -1, -1) if i != info.eos_id][:3]
    return blobs, ids, info.eos_id, sent


def segments(ids, rate, spm, sent, min_ids=0, first=0):
    """Per record (segment without its eos or None when dropped, kind, a, b, n): the contract's draw
    and permutation; record i of the list has the index first + i."""
    pre_id, suf_id, mid_id = sent
    d = np.arange(len(ids), dtype=np.uint64) + np.uint64(first)
    z = np.zeros_like(d)
    x = np.stack(philox4x32_10(z, z + np.uint64(0x90000000), d & np.uint64(M32), d >> np.uint64(32), SEED & M32, SEED >> 32), 1)
    out = []
    for t, (x0, x1, x2, x3) in zip(ids, x.tolist()):
        t, n = list(t), len(t)
        if not pack_model.kept(n, min_ids):
            out.append((None, "dropped", 0, 0, n))
        elif x0 * 1000 >= rate << 32:
            out.append((t, "untouched", 0, 0, n))
        else:
            c1, c2 = x1 * (n + 1) >> 32, x2 * (n + 1) >> 32
            a, b = min(c1, c2), max(c1, c2)
            prefix, middle, suffix = t[:a], t[a:b], t[b:]
            if x3 * 1000 < spm << 32:
                out.append(([pre_id, suf_id] + suffix + [mid_id] + prefix + middle, "spm", a, b, n))
            else:
                out.append(([pre_id] + prefix + [suf_id] + suffix + [mid_id] + middle, "psm", a, b, n))
    return out


def model(segs, S, eos, carry=pack_model.EMPTY):
    return pack_model.pack([s[0] for s in segs if s[0] is not None], S, eos, 0, carry)


def with_flush(want, S):
    return [np.concatenate([want[k], f]) for k, f in enumerate(pack_model.flush(want[4], S))]


def fim_packer(S, fim, min_ids=0):
    return DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=S, min_ids=min_ids, seed=SEED,
                         tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1, fim=fim)


def rows_of(torch, db, calls, S):
    """The rows of the calls and the flush, concatenated per plane, and the calls' d_record_rows."""
    got, rec = [[] for _ in NAMES], []
    for blobs in calls:
        res = run(torch, db, blobs)
        rec.append(res.record_rows())
        for k, plane in enumerate(four(res)):
            got[k].append(plane)
    fl = db.flush_device()
    torch.cuda.synchronize()
    for k, plane in enumerate(four(fl)):
        got[k].append(plane)
    return [np.concatenate(g) for g in got], np.concatenate(rec)


@pytest.mark.parametrize("rate,spm", [(1000, 0), (1000, 1000), (500, 500)])
@pytest.mark.parametrize("S", [30, 33, 64])
def test_one_call_then_flush(torch, native_lib, corpus, S, rate, spm):
    blobs, ids, eos, sent = corpus
    segs = segments(ids, rate, spm, sent)
    # conditions on the inputs: every kind the setting can give, and the empty prefix / suffix / middle
    kinds = {s[1] for s in segs}
    assert kinds >= {"dropped"} | ({"untouched"} if rate < 1000 else set()) | ({"psm"} if spm < 1000 else set()) | \
        ({"spm"} if spm > 0 else set())
    cut = [s for s in segs if s[1] in ("psm", "spm")]
    assert any(a == 0 for _, _, a, b, n in cut) and any(b == n for _, _, a, b, n in cut) and any(a == b for _, _, a, b, n in cut)
    assert max(len(s[0]) for s in cut) > 3 * S  # a transformed document over several rows
    want = model(segs, S, eos)
    db = fim_packer(S, B.Fim(rate, spm, *sent))
    got, rec = rows_of(torch, db, [blobs], S)
    db.close()
    check(got, with_flush(want, S), f"S={S} rate={rate} spm={spm}")
    np.testing.assert_array_equal(rec, [0 if s[0] is None else len(s[0]) + 1 for s in segs])


def test_split_invariance(torch, native_lib, corpus):
    """Three uneven calls and a flush give the rows of one call and a flush; the second call ends
    inside a transformed document, which finishes from the carry."""
    S, rate, spm = 33, 700, 400
    blobs, ids, eos, sent = corpus
    segs = segments(ids, rate, spm, sent)
    ends = np.cumsum([0 if s[0] is None else len(s[0]) + 1 for s in segs])

    def cut_inside(k):  # records [0, k): the last one is transformed and a row end falls inside its segment
        return segs[k - 1][1] in ("psm", "spm") and 0 < ends[k - 1] % S < len(segs[k - 1][0]) + 1
    k1 = next(k for k in range(40, len(ids)) if cut_inside(k))
    cuts = [0, 3, k1, len(ids)]
    want = model(segs, S, eos)
    db = fim_packer(S, B.Fim(rate, spm, *sent))
    got, rec = rows_of(torch, db, [blobs[a:b] for a, b in zip(cuts[:-1], cuts[1:])], S)
    db.close()
    check(got, with_flush(want, S), "three calls")
    np.testing.assert_array_equal(rec, [0 if s[0] is None else len(s[0]) + 1 for s in segs])


def test_rate_0_is_plain_pack(torch, native_lib, corpus):
    S = 33
    blobs, ids, eos, sent = corpus
    want = with_flush(pack_model.pack(ids, S, eos, 0), S)
    for fim in (B.Fim(0, 500, *sent), None):  # through the fill-in-the-middle kernels, and a handle that never calls set_fim
        db = fim_packer(S, fim)
        got, rec = rows_of(torch, db, [blobs], S)
        db.close()
        check(got, want, f"fim={fim}")
        np.testing.assert_array_equal(rec, pack_model.record_rows(ids, 0))


def test_host_path_batches(native_lib, records, oracle_gpt2, corpus):
    """GenTokenizer(Gpt(pack=True, fim=...)), B = 4, S = 64: two bulk pushes, then get_working_batch
    until None; the batches are the model's rows (flush row included) cut into groups of 4."""
    Bsz, S = 4, 64
    _, _, eos, sent = corpus
    ids = [oracle_gpt2.encode(t) for t in records]
    want = with_flush(model(segments(ids, 500, 500, sent, min_ids=64), S, eos), S)  # (GenTokenizer keeps the reference's min_ids)
    gt = B.GenTokenizer(B.ModelType.Gpt2, B.BatchConfig(Bsz, S), B.Gpt(pack=True, fim=B.Fim(500, 500, *sent)),
                        B.TokenizerConfig(native.GPT2_PROXY_TOKENIZER), chunk=True, seed=SEED)
    h = len(records) // 3
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


def test_refusals(torch, native_lib, corpus):
    blobs, _, eos, sent = corpus
    vocab = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER).vocab_size

    def refused(db, fim, code, word):
        assert native_lib.sdl_batcher_set_fim(db._h, ctypes.byref(fim)) == code
        assert word in native_lib.sdl_last_error().decode()
    ok = native.Fim(500, 500, *sent)
    plain = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=4, sequence_length=64, tokenizer=native.GPT2_PROXY_TOKENIZER)
    refused(plain, ok, -6, "pack = 1")  # SDL_ERR_STATE: not a packed clm handle
    plain.close()
    db = fim_packer(64, None)
    for field, value in [("rate_per_mille", 1001), ("spm_per_mille", -1), ("prefix_id", vocab), ("suffix_id", -1),
                         ("middle_id", eos), ("middle_id", sent[0])]:
        bad = native.Fim(500, 500, *sent)
        setattr(bad, field, value)
        refused(db, bad, -1, field)  # SDL_ERR_ARG, naming the field
    bad = native.Fim(500, 500, *sent)
    bad.reserved[2] = 1
    refused(db, bad, -1, "reserved")
    assert native_lib.sdl_batcher_set_fim(db._h, ctypes.byref(ok)) == 0  # still fresh: accepted
    run(torch, db, blobs[:2])
    refused(db, ok, -6, "seen a record")  # SDL_ERR_STATE
    db.close()
