"""Packed span rows on the device (sdl_config.pack = 1 under the span task, pack_span.hip): all three
planes of every row, exactly, against the model of the contract (tests/pack_span_model.py) over the
oracle Unigram tokenizer's ids of the fixture records -- one call and the flush row per case, calls
of uneven size, the host path's batch queue, the frames.  Each case's model rows are made once."""
import functools

import numpy as np
import pytest

import oracle_lib
import pack_span_model as model
import span_noise_model as M
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_parity import run_device, torch  # noqa: F401

pytestmark = pytest.mark.gpu
SEED, BSZ = 4321, 4
KEYS = ("input_ids", "attention_mask", "labels")

# (S, per mille, mean, min_ids): the label row filled exactly (N = 71); a width off the 4-int grid
# (N = 36); N = S and one span a row; mean 1.0 -- 150 per mille needs 39 of 32 labels at S = 128, 121
# is the densest word that fits (31 of 32); the filter dropping records; N = 1138 -- several key
# rounds, more than 256 Philox blocks over both domains; N = 2226, 90 sentinels, two waves a block
CASES = [(64, 150, 3.0, 0), (33, 100, 3.0, 0), (64, 1, 3.0, 0), (128, 121, 1.0, 0), (300, 150, 3.0, 64),
         (1024, 150, 3.0, 0), (2048, 120, 3.0, 0)]


@functools.lru_cache(maxsize=None)
def corpus():
    """(texts, ids per record): the fixture records with empty and short records among them."""
    texts = ("the",) + M.fixture_records()[:20] + ("", "the of and", "a", "") + M.fixture_records()[20:] + ("", "to be or not")
    return texts, tuple(tuple(M.tok().encode(t)[:-1]) for t in texts)  # (encode ends with the template's </s>)


@functools.lru_cache(maxsize=None)
def want(S, per_mille, mean, min_ids):
    """The model's rows of one call over the corpus, its carry and the flush row behind them."""
    _, ids = corpus()
    rows, carry = model.pack(ids, S, per_mille, mean, SEED, min_ids)
    fl = model.flush(carry, S, per_mille, mean, SEED, rows[0].shape[0])
    assert rows[0].shape[0] >= 2 and len(carry) > 0 and fl[0].shape[0] == 1, (S, rows[0].shape, len(carry))
    for a in rows + fl:
        a.setflags(write=False)
    return rows, fl


def packer(S, per_mille, mean, min_ids):
    return DeviceBatcher(task=native.SDL_TASK_SPAN, batch_size=BSZ, sequence_length=S, seed=SEED, min_ids=min_ids,
                         tokenizer=native.T5_PROXY_TOKENIZER, avg_span_size=mean, span_policy=1,
                         span_noise_per_mille=per_mille, pack=1)


def three(res, n=None):
    ids, am, tt, lab = res.planes(n)
    assert tt is None and res.position_ids(n) is None and lab.shape[1] == ids.shape[1] // 4
    assert res.label_errors() == 0 and res.tokenize_errors() == 0
    return ids, am, lab


def check(got, wanted, what):
    for k, g, w in zip(KEYS, got, wanted):
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {k}")


def check_padding(res, G):
    n = -(-G // BSZ) * BSZ
    if n > G:  # T5Data::new's values
        ids, am, lab = three(res, n)
        assert (ids[G:] == 0).all() and (am[G:] == 1).all() and (lab[G:] == -100).all()


@pytest.mark.parametrize("S,per_mille,mean,min_ids", CASES)
def test_one_call_then_flush(torch, native_lib, S, per_mille, mean, min_ids):  # noqa: F811
    texts, ids = corpus()
    rows, fl = want(S, per_mille, mean, min_ids)
    G, N = rows[0].shape[0], model.chunk_length(S, per_mille, mean)
    rr = model.record_rows(ids, min_ids)
    assert (rr == 0).sum() > (3 if min_ids == 0 else 5)  # the empty records; under min_ids also short ones
    if (S, per_mille) == (64, 150):
        assert (rows[2][:, -1] != -100).all()  # the label row filled exactly
    db = packer(S, per_mille, mean, min_ids)
    assert native_lib.sdl_pack_span_length(db.cfg) == N
    res = run_device(torch, db, list(texts))
    assert res.rows() == G
    assert res.r.rows_capacity >= -(-G // BSZ) * BSZ and res.r.rows_capacity % BSZ == 0
    check(three(res), rows, f"S={S} {per_mille}/{mean} min_ids={min_ids}")
    check_padding(res, G)
    np.testing.assert_array_equal(res.record_rows(), rr)
    f = db.flush_device()
    torch.cuda.synchronize()
    assert f.rows() == 1
    check(three(f), fl, f"S={S} flush")
    check_padding(f, 1)
    assert db.flush_device().rows() == 0
    db.close()


def test_uneven_calls_equal_one_call(torch, native_lib):  # noqa: F811
    """An R = 0 call, a one-record call that emits no row, an R = 0 call with a carry waiting, then
    calls of uneven size: row for row the rows of one call over all records, flush row included."""
    S, per_mille, mean = 64, 150, 3.0
    texts, ids = corpus()
    rows, fl = want(S, per_mille, mean, 0)
    n = len(texts)
    cuts = [0, 0, 1, 1, 7, 13, 14, n - 3, n]
    db = packer(S, per_mille, mean, 0)
    got, rr = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        res = run_device(torch, db, list(texts[a:b]))
        G = res.rows()
        assert (a, b) != (0, 1) or G == 0
        got.append(three(res, G))
        rr.append(res.record_rows())
        check_padding(res, G)
    f = db.flush_device()
    torch.cuda.synchronize()
    got.append(three(f))
    check([np.concatenate(p) for p in zip(*got)], [np.concatenate(p) for p in zip(rows, fl)], f"calls {cuts}")
    np.testing.assert_array_equal(np.concatenate(rr), model.record_rows(ids, 0))
    db.close()


def test_host_path_batches(native_lib):
    """GenTokenizer(Span(pack=True)), B = 4, S = 64: per-record pushes, then get_working_batch until
    None; the batches are the model's rows (flush row included) cut into groups of 4."""
    S = 64
    texts, _ = corpus()
    rows, fl = want(S, 150, 3.0, 64)  # (GenTokenizer keeps the reference's min_ids)
    wanted = [np.concatenate(p) for p in zip(rows, fl)]
    n = wanted[0].shape[0]
    gt = B.GenTokenizer(B.ModelType.T5, B.BatchConfig(BSZ, S), B.Span(16.0, 3.0, policy=1, noise_per_mille=150, pack=True),
                        B.TokenizerConfig(native.T5_PROXY_TOKENIZER), chunk=True, seed=SEED)
    got = [b for b in (gt.create_sync_batch(t) for t in texts) if b is not None]
    while True:
        b = gt.get_working_batch()
        if b is None:
            break
        got.append(b)
    assert len(got) == -(-n // BSZ) and sum(b.rows for b in got) == n
    for i, ds in enumerate(got):
        d = ds.to_dict()
        assert set(d) == set(KEYS) and ds.token_type_ids is None
        for k, w in zip(KEYS, wanted):
            np.testing.assert_array_equal(d[k][:ds.rows], w[i * BSZ:i * BSZ + ds.rows], err_msg=f"batch {i} {k}")
    gt.close()


def test_frames_of_a_packed_call(torch, native_lib):  # noqa: F811
    """sdl_pickle_frames_device over a packed call's rows: the three span keys, packed planes."""
    S = 64
    texts, _ = corpus()
    rows, _ = want(S, 150, 3.0, 0)
    full = M.padded(dict(zip(KEYS, rows)), BSZ)
    db = packer(S, 150, 3.0, 0)
    res = run_device(torch, db, list(texts))
    n = res.rows()
    assert n == rows[0].shape[0] and n > BSZ
    frames = db.pickle_frames(res, n, flush_partial=True).frames()
    assert len(frames) == -(-n // BSZ)
    for f, frame in enumerate(frames):
        sl = slice(f * BSZ, (f + 1) * BSZ)
        assert frame == oracle_lib.pickle_dataset("span", BSZ, S, S // 4, min(BSZ, n - f * BSZ), full["input_ids"][sl],
                                                  full["attention_mask"][sl], None, full["labels"][sl]), f
    db.close()
