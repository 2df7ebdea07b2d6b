"""Row, copy-out and frame kernels at row widths off the 4-int grid.

Every kernel that writes a [rows, S] or [rows, label_width] plane has a 16-byte path (width a
multiple of 4 ints) and a scalar one: rows_device.hpp store4 (row_one, row_policy_one),
pipeline.hip span_plane, k_rows_to_host and k_rows_direct, transport_frame.hip k_frame_rows
(the k0 + 4 > W tail, the loads of runs that do not start 16-byte aligned).  The widths here
take the scalar ones: every S & 3 in {1, 2, 3}, fewer than one quad per lane, one element on
either side of each MR = ceil(S / 256) instantiation, and the largest width below the limit.
Span label widths S / 4 that are again multiples of 4 (S = 65, 257, 513, 1025) keep the 16-byte
label stores beside scalar id stores; in a host batch such a label plane does not start
16-byte aligned when B is odd.

Everything is bit-exact against the C oracle (rows) or the pickle oracle (frames); each test
asserts that its input reached what it is about (masked labels, full and short rows, pad rows).
"""
import functools
import json
import os
import pickle

import numpy as np
import pytest

import oracle_lib
from streaming_data_loader_amd import batcher as Bt
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_gpt2 import hard_blobs as gpt2_hard_blobs
from test_gpu_parity import hard_records as bert_hard_records
from test_gpu_span import hard_blobs as t5_hard_blobs
from test_pickle_frames import want_dict

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WIDTHS = (5, 7, 63, 65, 127, 254, 257, 513, 1023, 1025, 2047)
HOST_WIDTHS = (7, 65, 127, 257, 1023)
SEED, FIRST = 4321, 3
NL = 9
INT_KEYS = ("input_ids", "attention_mask", "token_type_ids", "labels")
TASK = {"mlm": (oracle_lib.MLM, native.SDL_TASK_MLM, "bert"), "clm": (oracle_lib.CLM, native.SDL_TASK_CLM, "gpt2"),
        "span": (oracle_lib.SPAN, native.SDL_TASK_SPAN, "t5"),
        "multi-label": (oracle_lib.MULTI_LABEL, native.SDL_TASK_MULTI_LABEL, "bert"),
        "single-class": (oracle_lib.SINGLE_CLASS, native.SDL_TASK_SINGLE_CLASS, "bert")}
TOKENIZER = {"bert": native.BERT_PROXY_TOKENIZER, "gpt2": native.GPT2_PROXY_TOKENIZER,
             "t5": native.T5_PROXY_TOKENIZER}
# the pad rows of a last batch (BertData::new / GptData::new / T5Data::new; the multi-hot and
# the single-class label of a row nobody filled are 0: k_multi_labels, k_single_labels)
PAD_LABEL = {"mlm": -100, "clm": -100, "span": -100, "multi-label": 0, "single-class": 0}


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


def mask_length_of(S):
    return max(1, int(S * 0.15))  # (the default, (S as f32 * 0.15) as usize, is 0 at S = 5)


# ---- inputs ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_texts():
    with open(os.path.join(GOLDEN, "test_records.jsonl"), encoding="utf-8") as f:
        return tuple(json.loads(l)["text"] for l in f)


@functools.lru_cache(maxsize=None)
def short_hard(tok):
    """A handful of short records from the tokenizer tests' hard lists (each list is pinned to
    its oracle by the tokenizer's own GPU test)."""
    if tok == "bert":
        pool = [t.encode("utf-8") for t in bert_hard_records(3)]
    else:
        pool = (gpt2_hard_blobs if tok == "gpt2" else t5_hard_blobs)(13, 120)
    return tuple(b for b in pool if 0 < len(b) <= 160)[:8]


@functools.lru_cache(maxsize=None)
def blobs_for(tok, S, drop=0):
    """The first records of the fixture (fewer at S <= 7: under ~2000 rows) less the last `drop`,
    short hard records between them and, from S = 513 on, one record long enough to fill whole
    rows."""
    texts = fixture_texts()
    recs = [t.encode("utf-8") for t in texts[:(16 if S <= 7 else 30) - drop]]
    if S >= 513:
        recs.insert(5, " ".join(texts[20:34]).encode("utf-8"))
    out = []
    hard = list(short_hard(tok))
    for i, r in enumerate(recs):
        out.append(r)
        if i % 3 == 1 and hard:
            out.append(hard.pop())
    out.insert(4, b"a")  # (rows shorter than S = 5: one id and no id inside the framing)
    out.append(b"")
    return tuple(out)


@functools.lru_cache(maxsize=None)
def label_sets(n, single):
    rng = np.random.default_rng(n)
    if single:
        return tuple((int(rng.integers(0, 2)),) for _ in range(n))
    return tuple(tuple(int(x) for x in rng.choice(NL, size=rng.integers(0, 4), replace=False)) for _ in range(n))


# ---- the oracle -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encoder(tok):
    t = {"bert": oracle_lib.Tok, "gpt2": oracle_lib.Gpt2Tok, "t5": oracle_lib.T5Tok}[tok]()
    return oracle_lib.Encoder(tok, t)


def oracle_batcher(task, B, S, rng_mode=0, gap=16.0, size=2.0, min_ids=0):
    ob = oracle_lib.OracleBatcherEx(encoder(TASK[task][2]), TASK[task][0], B, S, mask_length=mask_length_of(S),
                                    number_labels=NL, seed=SEED, min_ids=min_ids, avg_span_gap=gap,
                                    avg_span_size=size, rng_mode=rng_mode)
    ob.set_next_record(FIRST)
    return ob


def oracle_batches(ob, task, blobs, labels=None):
    """Every batch the reference Batcher emits for `blobs`, in order: one push per record, then
    the flushes (SimpleBatcher's flush always returns a batch: once)."""
    want = [r for r in (ob.push(b, None if labels is None else labels[i]) for i, b in enumerate(blobs))
            if r is not None]
    if task in ("multi-label", "single-class"):
        want.append(ob.flush())
    else:
        while True:
            r = ob.flush()
            if r is None:
                break
            want.append(r)
    return want


@functools.lru_cache(maxsize=None)
def oracle_rows(task, B, S, rng_mode=0, gap=16.0, size=2.0, drop=0):
    """(planes of all filled rows, span errors) of the reference Batcher over blobs_for()."""
    blobs = blobs_for(TASK[task][2], S, drop)
    labels = label_sets(len(blobs), task == "single-class") if task in ("multi-label", "single-class") else None
    ob = oracle_batcher(task, B, S, rng_mode, gap, size)
    want = oracle_batches(ob, task, blobs, labels)
    keys = INT_KEYS + (("labels_f32",) if task == "multi-label" else ())
    cat = {k: np.concatenate([w[k][:w["rows"]] for w in want]) for k in keys}
    if task == "multi-label":
        cat["labels"] = cat.pop("labels_f32")
    for a in cat.values():
        a.setflags(write=False)
    return cat, ob.span_errors()


def partial_batch_size(n_rows, candidates):
    """The first batch size that leaves the last batch partial."""
    return next(b for b in candidates if n_rows % b)


@functools.lru_cache(maxsize=None)
def row_lengths(tok, S):
    """Filled positions l of every row GenTokenizer cuts blobs_for(tok, S) into: the clm rows of
    the same tokenizer zero exactly l attention positions when l < S and none when l == S."""
    ob = oracle_lib.OracleBatcherEx(encoder(tok), oracle_lib.CLM, 64, S, seed=SEED, min_ids=0)
    want = oracle_batches(ob, "clm", blobs_for(tok, S))
    zeros = np.concatenate([(w["attention_mask"][:w["rows"]] == 0).sum(axis=1) for w in want])
    return np.where(zeros == 0, S, zeros)


def assert_exercised(task, S, B, want):
    """The guards against a vacuous case, on the oracle's rows."""
    G = want["input_ids"].shape[0]
    assert G > B and G % B != 0, f"{task} S={S}: {G} rows at B={B} leave no pad row"
    if task == "span":  # (T5Data never zeroes attention: the rows' lengths from the tokenizer)
        l = row_lengths("t5", S)
        assert l.size == G
        if S > 7:  # (a width-1 label row may stay empty)
            assert (want["labels"] != -100).any()
    else:
        zeros = (want["attention_mask"] == 0).sum(axis=1)
        l = np.where(zeros == 0, S, zeros)
    # (SimpleBatcher frames a record with five ids, [CLS] [CLS] .. [SEP] [SEP] [SEP]: no short row at S = 5)
    short = S > 5 or task not in ("multi-label", "single-class")
    assert (l < S).any() == short and (l == S).any(), \
        f"{task} S={S}: short rows {(l < S).sum()}, full rows {(l == S).sum()}"
    if task == "mlm":
        assert (want["labels"] != -100).any()
    if task == "multi-label":
        assert (want["labels"] == 1).any()


# ---- the device path ------------------------------------------------------------------------------
def to_device(torch, blobs):
    offs = np.zeros(len(blobs) + 1, np.int64)
    np.cumsum([len(b) for b in blobs], out=offs[1:])
    arena = np.zeros(int(offs[-1]) + 16, np.uint8)
    arena[:int(offs[-1])] = np.frombuffer(b"".join(blobs), np.uint8)
    return torch.from_numpy(arena).cuda(), torch.from_numpy(offs).cuda(), int(offs[-1])


def device_run(torch, task, B, S, rng_mode=0, gap=16.0, size=2.0, drop=0):  # noqa: F811
    """DeviceBatcher over blobs_for(): (handle, result); the caller closes the handle."""
    tok = TASK[task][2]
    blobs = blobs_for(tok, S, drop)
    db = DeviceBatcher(task=TASK[task][1], batch_size=B, sequence_length=S, mask_length=mask_length_of(S), seed=SEED,
                       tokenizer=TOKENIZER[tok], min_ids=0, number_labels=NL, avg_span_gap=gap, avg_span_size=size,
                       rng_mode=rng_mode)
    ta, to, n = to_device(torch, blobs)
    if task in ("multi-label", "single-class"):
        sets = label_sets(len(blobs), task == "single-class")
        lo = np.zeros(len(sets) + 1, np.int64)
        np.cumsum([len(s) for s in sets], out=lo[1:])
        vals = np.array([v for s in sets for v in s] + [0], np.int32)  # (never empty)
        tl, tlo = torch.from_numpy(vals).cuda(), torch.from_numpy(lo).cuda()
        res = db.process_labels(ta.data_ptr(), n, to.data_ptr(), len(blobs), tl.data_ptr(), tlo.data_ptr(), FIRST)
    else:
        res = db.process(ta.data_ptr(), n, to.data_ptr(), len(blobs), FIRST)
    torch.cuda.synchronize()
    return db, res


def assert_planes(task, S, B, res, want):
    """Every plane of every filled row bit-equal; the pad rows hold the initial values."""
    G = res.rows()
    assert G == want["input_ids"].shape[0]
    Gp = -(-G // B) * B
    assert Gp > G
    ids, am, tt, lab = res.planes(Gp)
    got = {"input_ids": ids, "attention_mask": am, "token_type_ids": tt, "labels": lab}
    if task in ("clm", "span"):
        assert tt is None
        del got["token_type_ids"]
    LW = {"span": S // 4, "multi-label": NL, "single-class": 1}.get(task, S)
    assert lab.shape == (Gp, LW) and lab.dtype == (np.float32 if task == "multi-label" else np.int32)
    for k, a in got.items():
        bad = np.nonzero((a[:G] != want[k]).any(axis=1))[0]
        assert bad.size == 0, f"{task} S={S}: {k}, {bad.size} of {G} rows differ, first {bad[:5]}"
    assert (ids[G:] == 0).all() and (am[G:] == 1).all() and (lab[G:] == PAD_LABEL[task]).all()
    assert tt is None or (tt[G:] == 0).all()
    return got


def check_device(torch, task, S, rng_mode=0, gap=16.0, size=2.0, span_errors=False):  # noqa: F811
    # (the rows do not depend on the batch size: the first of 7, 6, 5 that leaves pad rows)
    B = partial_batch_size(oracle_rows(task, 7, S, rng_mode, gap, size)[0]["input_ids"].shape[0], (7, 6, 5))
    want, errs = oracle_rows(task, B, S, rng_mode, gap, size)
    assert_exercised(task, S, B, want)
    db, res = device_run(torch, task, B, S, rng_mode, gap, size)
    assert_planes(task, S, B, res, want)
    if task == "span":
        assert (errs > 0) == span_errors and res.label_errors() == errs
    else:
        assert res.label_errors() == 0
    db.close()


@pytest.mark.parametrize("rng_mode", [0, 1])
@pytest.mark.parametrize("S", WIDTHS)
def test_mlm_rows(torch, native_lib, S, rng_mode):  # noqa: F811
    check_device(torch, "mlm", S, rng_mode)


@pytest.mark.parametrize("S", WIDTHS)
def test_clm_rows(torch, native_lib, S):  # noqa: F811
    check_device(torch, "clm", S)


@pytest.mark.parametrize("rng_mode,two_phase", [(0, False), (1, False), (0, True)])
@pytest.mark.parametrize("S", WIDTHS)
def test_span_rows(torch, native_lib, S, rng_mode, two_phase, monkeypatch):  # noqa: F811
    """One-pass and two-phase (k_span_plan + k_span_write) span rows; gap 16 / size 2 stays inside
    the S / 4 labels at these widths, so the error count is the oracle's 0 -- but for S = 2047,
    whose full rows ask for more than the 100 sentinels."""
    if two_phase:
        monkeypatch.setenv("SDL_SPAN_TWO_PHASE", "1")
    check_device(torch, "span", S, rng_mode, span_errors=S == 2047)


@pytest.mark.parametrize("S,gap,size", [(127, 3.0, 3.0), (17, 16.0, 2.0)])
def test_span_rows_past_the_label_width(torch, native_lib, S, gap, size):  # noqa: F811
    """The clamped writes at odd widths: gap 3 / size 3 at S = 127 overruns the 31 labels, the
    default gap the 4 labels of S = 17; the count of writes out of range is the oracle's."""
    check_device(torch, "span", S, 0, gap, size, span_errors=True)


@pytest.mark.parametrize("S", WIDTHS)
def test_multi_label_rows(torch, native_lib, S):  # noqa: F811
    check_device(torch, "multi-label", S)


@pytest.mark.parametrize("S", WIDTHS)
def test_single_class_rows(torch, native_lib, S):  # noqa: F811
    check_device(torch, "single-class", S)


# ---- the host path --------------------------------------------------------------------------------
def host_batcher(task, B, S, rng_mode=0):
    model, cfg = {"mlm": (Bt.ModelType.Bert, Bt.Mask(mask_length_of(S), 103)), "clm": (Bt.ModelType.Gpt2, Bt.Gpt()),
                  "span": (Bt.ModelType.T5, Bt.Span(16.0, 2.0))}[task]
    return Bt.GenTokenizer(model, Bt.BatchConfig(B, S), cfg, Bt.TokenizerConfig(TOKENIZER[TASK[task][2]]), chunk=True,
                           seed=SEED, first_record=FIRST, rng_mode=rng_mode)


def drain(gt, got):
    while True:
        d = gt.get_working_batch()
        if d is None:
            return got
        got.append(d)


def assert_batches(task, S, got, want):
    assert [d.rows for d in got] == [w["rows"] for w in want]
    for i, (d, w) in enumerate(zip(got, want)):
        n = w["rows"]
        for k in INT_KEYS:
            a = getattr(d, k)
            if task != "mlm" and k == "token_type_ids":
                assert a is None
                continue
            np.testing.assert_array_equal(a[:n], w[k][:n], err_msg=f"{task} S={S} batch {i} {k}")
        # rows nobody filled: the initial values
        assert (d.input_ids[n:] == 0).all() and (d.attention_mask[n:] == 1).all() and (d.labels[n:] == -100).all()


@pytest.mark.parametrize("task,rng_mode", [("mlm", 0), ("mlm", 1), ("clm", 0), ("span", 0)])
@pytest.mark.parametrize("S", HOST_WIDTHS)
def test_host_batches(native_lib, S, task, rng_mode):
    """GenTokenizer record by record (small pushes: row_one / k_rows_direct write the pinned
    batches, rows past the two open batches go through k_rows_to_host) and the same records in
    one push_many: batch by batch the oracle's pushes and flushes.  B is odd, so the label plane
    of a host batch starts 8 bytes off the 16-byte grid at odd S."""
    blobs = blobs_for(TASK[task][2], S)
    B = partial_batch_size(sum(w["rows"] for w in oracle_batches(oracle_batcher(task, 3, S, rng_mode, min_ids=64),
                                                                 task, blobs)), (3, 5, 7))
    ob = oracle_batcher(task, B, S, rng_mode, min_ids=64)
    want = oracle_batches(ob, task, blobs)
    assert ob.span_errors() == 0  # (nothing for the host path to refuse)
    rows = sum(w["rows"] for w in want)
    assert len(want) > 2 and rows % B != 0
    cat = {k: np.concatenate([w[k][:w["rows"]] for w in want]) for k in INT_KEYS}
    zeros = (cat["attention_mask"] == 0).sum(axis=1)
    if task != "span":
        assert (zeros > 0).any() and (zeros == 0).any()
    if task != "clm" and S > 7:
        assert (cat["labels"] != -100).any()
    one = host_batcher(task, B, S, rng_mode)
    per = drain(one, [d for d in (one.create_sync_batch(b) for b in blobs) if d is not None])
    assert_batches(task, S, per, want)
    many = host_batcher(task, B, S, rng_mode)
    bulk = drain(many, many.create_sync_batches(list(blobs)))
    assert_batches(task, S, bulk, want)
    one.close()
    many.close()


def test_host_span_refused_where_the_reference_panics(native_lib):
    """S = 17: the default gap overruns the 4 labels; the host path fails the call."""
    blobs = blobs_for("t5", 17)
    ob = oracle_batcher("span", 3, 17, min_ids=64)
    oracle_batches(ob, "span", blobs)
    assert ob.span_errors() > 0
    gt = host_batcher("span", 3, 17)
    with pytest.raises(native.SDLError, match="reference panics"):
        for b in blobs:
            gt.create_sync_batch(b)
    gt.close()


@pytest.mark.parametrize("n_labels", [9, 8])
def test_host_multi_label(native_lib, n_labels):
    """SimpleBatcher at S = 65, B = 3, per record and in one call (8 labels: a label plane whose
    rows are a multiple of 16 bytes and whose start in the host batch is not)."""
    S, B = 65, 3
    blobs = blobs_for("bert", S)
    sets = [[v for v in s if v < n_labels] for s in label_sets(len(blobs), False)]
    ob = oracle_lib.OracleBatcherEx(encoder("bert"), oracle_lib.MULTI_LABEL, B, S, number_labels=n_labels)
    want = oracle_batches(ob, "multi-label", blobs, sets)
    assert len(want) > 2 and 0 < want[-1]["rows"] < B
    items = [Bt.SimpleTransport(Bt.SimpleData(b), Bt.Label(multi=s)) for b, s in zip(blobs, sets)]

    def check(got):
        assert [d.rows for d in got] == [w["rows"] for w in want]
        for i, (d, w) in enumerate(zip(got, want)):
            for k in ("input_ids", "attention_mask", "token_type_ids"):
                np.testing.assert_array_equal(getattr(d, k), w[k], err_msg=f"batch {i} {k}")
            assert d.labels.dtype == np.float32 and d.labels.shape == (B, n_labels)
            np.testing.assert_array_equal(d.labels, w["labels_f32"], err_msg=f"batch {i} labels")
    one = Bt.SimpleBatcher(Bt.ModelType.Bert, Bt.MultiLabel(n_labels), Bt.BatchConfig(B, S), Bt.TokenizerConfig())
    check([d for d in (one.create_sync_batch(t) for t in items) if d is not None] + [one.get_working_batch()])
    many = Bt.SimpleBatcher(Bt.ModelType.Bert, Bt.MultiLabel(n_labels), Bt.BatchConfig(B, S), Bt.TokenizerConfig())
    check(many.create_sync_batches(items) + [many.get_working_batch()])
    one.close()
    many.close()


# ---- the transport frames -------------------------------------------------------------------------
# mlm 1003 x 5: more than 1000 rows a frame (an APPENDS marker between runs) at 200 rows a wave;
# clm 130 x 7: more than one 125-row run; clm 2 x 2047: two inner markers; span 8 x 101 / 5 x 127:
# label widths 25 / 31
FRAME_CASES = [("mlm", 3, 5), ("mlm", 1003, 5), ("mlm", 8, 127), ("mlm", 4, 1023), ("clm", 130, 7), ("clm", 3, 1001),
               ("clm", 2, 2047), ("span", 8, 101), ("span", 5, 127), ("multi-label", 7, 65)]


@pytest.mark.parametrize("task,B,S", FRAME_CASES)
def test_frames(torch, native_lib, task, B, S):  # noqa: F811
    # (the issue's B and S; the fixture less 0, 1 or 2 records, so that the last batch is partial)
    drop = next(d for d in (0, 1, 2) if oracle_rows(task, B, S, drop=d)[0]["input_ids"].shape[0] % B)
    want, _ = oracle_rows(task, B, S, drop=drop)
    db, res = device_run(torch, task, B, S, drop=drop)
    n = res.rows()
    assert n == want["input_ids"].shape[0] and n > B and n % B != 0
    for flush in (True, False):
        fr = db.pickle_frames(res, n, flush_partial=flush)
        torch.cuda.synchronize()
        nb = n // B + (1 if flush else 0)
        assert len(fr) == nb  # (n > B: at least one full frame, and the partial one when flushed)
        frames = fr.frames()
        ids, am, tt, lab = res.planes(nb * B)
        for k, a in (("input_ids", ids), ("attention_mask", am), ("labels", lab)):
            m = min(n, nb * B)
            np.testing.assert_array_equal(a[:m], want[k][:m], err_msg=f"{task} {B}x{S} {k}")
        for b, frame in enumerate(frames):
            rows = min(B, n - b * B)
            sl = slice(b * B, (b + 1) * B)
            ref = oracle_lib.pickle_dataset(task, B, S, lab.shape[1], rows, ids[sl], am[sl],
                                            None if tt is None else tt[sl], lab[sl])
            assert len(frame) == len(ref), f"{task} {B}x{S} frame {b}: {len(frame)} bytes for {len(ref)}"
            assert frame == ref, f"{task} {B}x{S} frame {b}: first difference at byte " \
                                 f"{next(i for i, (x, y) in enumerate(zip(frame, ref)) if x != y)}"
        sl = slice((nb - 1) * B, nb * B)
        rows = min(B, n - (nb - 1) * B)
        assert pickle.loads(frames[-1]) == want_dict(task, rows, ids[sl], am[sl], None if tt is None else tt[sl],
                                                     lab[sl])
    db.close()
