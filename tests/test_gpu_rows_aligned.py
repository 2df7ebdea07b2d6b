"""The rows kernels at row widths on the 4-int grid: what launch_rows sends to the lean kernels
(pipeline.hip k_rows_fast, rows_device.hpp row_fast_one) -- S a multiple of 4, device planes, the
Philox contract -- and, beside them, the calls at the same widths that keep k_rows (per-record
pushes into host batches, rng_mode 1).

Widths: every 256 MR and its neighbours +-4, and 8 / 64 / 128.  Tasks mlm, clm, multi-label and
single-class; the WordPiece tasks from the dense id array (a call of at most 64 chunks) and from
the chunk lists (more than 64 chunks, 100-400 KiB).  Row forms at S = 8, 256 and 512: records
whose framed length is k S, k S + 1 (a row that holds only the closing frame) and k S - 1, short
final rows, records under the min_ids filter, a last record whose ids end in the arena's last
chunk, a last batch with padding rows -- each asserted on the oracle's side before the compare.

Every row of every plane is compared bit-exactly with the CPU oracle.  The helpers are those of
test_gpu_odd_widths.py and test_gpu_rows_from_lists.py."""
import functools

import numpy as np
import pytest

import oracle_lib
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_odd_widths import (FIRST, INT_KEYS, NL, SEED, TASK, TOKENIZER, assert_batches, assert_planes, drain,
                                 encoder, fixture_texts, host_batcher, label_sets, mask_length_of, oracle_batcher,
                                 oracle_batches, partial_batch_size, short_hard, to_device, torch)  # noqa: F401
from test_gpu_parity import run_device
from test_gpu_rows_from_lists import FILLER

pytestmark = pytest.mark.gpu

CHUNK = 1024
WIDTHS = (8, 64, 128, 252, 256, 260, 508, 512, 516, 1020, 1024, 1028, 2048)
FORM_WIDTHS = (8, 256, 512)
MIN_IDS = 12  # (the form arenas: records of fewer framed ids are dropped)
SEP = 102
FRAME = 5  # the Batcher's BERT framing: [CLS] [CLS] ids [SEP] [SEP] [SEP]


def n_chunks(blobs):
    return -(-sum(len(b) for b in blobs) // CHUNK)


# ---- inputs ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blobs_for(tok, lists):
    """Fixture records with short hard records between them, an empty record and a one-byte one:
    under 64 chunks (the dense id array), or -- lists -- the fixture over again up to 130 KiB."""
    texts = [t.encode("utf-8") for t in fixture_texts()]
    hard = list(short_hard(tok))
    long = b" ".join(texts[20:34])[:12000 if not lists else 28000]  # (full rows at S = 2048)
    long = long.decode("utf-8", "ignore").encode("utf-8")
    out, size, i = [], len(long), 0
    limit = (130 << 10) if lists else (56 << 10)
    while size + len(texts[i % len(texts)]) <= limit:
        out.append(texts[i % len(texts)])
        size += len(out[-1])
        if i % 3 == 1 and hard:
            out.append(hard.pop())
            size += len(out[-1])
        i += 1
    out.insert(5, long)
    out.insert(4, b"a")
    out.insert(9, b"")
    out = tuple(out)
    assert (n_chunks(out) > 64 and 100 << 10 <= size <= 400 << 10) if lists else n_chunks(out) <= 64
    return out


@functools.lru_cache(maxsize=None)
def form_blobs(S, lists):
    """WordPiece records of known id counts ('!' is one id, the framing FRAME more) for the row
    forms, filler records between them; the first record and the last one are kept by the filter,
    and the last one's ids reach the arena's last chunk."""
    rng = np.random.default_rng(S)

    def filler(n):
        return " ".join(FILLER[int(x)] for x in rng.integers(0, len(FILLER), n)).encode()

    def bangs(framed):
        return b"!" * (framed - FRAME)
    out = [filler(40)]
    for k in (1, 2, 5):
        for d in (0, 1, -1):
            if k * S + d > FRAME:
                out += [bangs(k * S + d), filler(int(rng.integers(1, 7)))]  # (fillers under the filter)
    out += [b"", bangs(MIN_IDS - 1), bangs(MIN_IDS), b"!"]  # ("" and "!": 5 and 6 framed ids)
    size = sum(len(b) for b in out)
    limit = (110 << 10) if lists else (40 << 10)
    while size < limit:
        out.append(filler(int(rng.integers(20, 700))))
        size += len(out[-1])
    out.append(bangs(2 * S + S // 2))  # the last record: a short final row, ids in the last chunk
    out = tuple(out)
    assert n_chunks(out) > 64 if lists else n_chunks(out) <= 64
    return out


def framed_lengths(blobs):
    tok = encoder("bert").tok  # (encode frames the ids itself, with one [CLS] and one [SEP])
    return np.array([len(tok.encode(b.decode("utf-8"))) - 2 + FRAME for b in blobs])


# ---- oracle and device ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_planes(task, S, blobs, rng_mode=0, min_ids=0):
    labels = label_sets(len(blobs), task == "single-class") if task in ("multi-label", "single-class") else None
    B = 7
    want = oracle_batches(oracle_batcher(task, B, S, rng_mode, min_ids=min_ids), task, blobs, labels)
    keys = INT_KEYS + (("labels_f32",) if task == "multi-label" else ())
    cat = {k: np.concatenate([w[k][:w["rows"]] for w in want]) for k in keys}
    if task == "multi-label":
        cat["labels"] = cat.pop("labels_f32")
    for a in cat.values():
        a.setflags(write=False)
    return cat


def device_planes(torch, task, B, S, blobs, rng_mode=0, min_ids=0):  # noqa: F811
    tok = TASK[task][2]
    db = DeviceBatcher(task=TASK[task][1], batch_size=B, sequence_length=S, mask_length=mask_length_of(S), seed=SEED,
                       tokenizer=TOKENIZER[tok], min_ids=min_ids, number_labels=NL, rng_mode=rng_mode)
    ta, to, n = to_device(torch, blobs)
    if task in ("multi-label", "single-class"):
        sets = label_sets(len(blobs), task == "single-class")
        lo = np.zeros(len(sets) + 1, np.int64)
        np.cumsum([len(s) for s in sets], out=lo[1:])
        vals = np.array([v for s in sets for v in s] + [0], np.int32)
        tl, tlo = torch.from_numpy(vals).cuda(), torch.from_numpy(lo).cuda()
        res = db.process_labels(ta.data_ptr(), n, to.data_ptr(), len(blobs), tl.data_ptr(), tlo.data_ptr(), FIRST)
    else:
        res = db.process(ta.data_ptr(), n, to.data_ptr(), len(blobs), FIRST)
    torch.cuda.synchronize()
    return db, res


def check(torch, task, S, blobs, rng_mode=0, min_ids=0):  # noqa: F811
    want = oracle_planes(task, S, blobs, rng_mode, min_ids)
    G = want["input_ids"].shape[0]
    B = partial_batch_size(G, (7, 6, 5))  # (the rows do not depend on the batch size)
    assert G > B
    zeros = (want["attention_mask"] == 0).sum(axis=1)
    assert (zeros > 0).any() and (zeros == 0).any(), f"{task} S={S}: short rows {(zeros > 0).sum()} of {G}"
    if task == "mlm":
        assert (want["labels"] != -100).any()
    db, res = device_planes(torch, task, B, S, blobs, rng_mode, min_ids)
    assert_planes(task, S, B, res, want)
    assert res.label_errors() == 0
    db.close()
    return want


# ---- every width, task and id source --------------------------------------------------------------
@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("task", ["mlm", "multi-label", "single-class"])
@pytest.mark.parametrize("S", WIDTHS)
def test_wordpiece_rows(torch, native_lib, S, task, lists):  # noqa: F811
    check(torch, task, S, blobs_for("bert", lists))


@pytest.mark.parametrize("S", WIDTHS)
def test_clm_rows(torch, native_lib, S):  # noqa: F811
    """gpt2 BPE: the dense id array at every size of call."""
    check(torch, "clm", S, blobs_for("gpt2", False))


# ---- the row forms --------------------------------------------------------------------------------
@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("S", FORM_WIDTHS)
def test_row_forms(torch, native_lib, S, lists):  # noqa: F811
    blobs = form_blobs(S, lists)
    n = framed_lengths(blobs)
    kept = n >= MIN_IDS
    assert (n[kept] % S == 0).any() and (n[kept] % S == 1).any() and (n[kept] % S == S - 1).any()
    assert (~kept).any() and kept[0] and kept[-1] and len(blobs[-1]) > 0
    assert 1 < n[-1] % S < S  # (the last row: short, with ids of the arena's last chunk)
    want = check(torch, "mlm", S, blobs, min_ids=MIN_IDS)
    G = want["input_ids"].shape[0]
    assert G == int(np.sum(-(-n[kept] // S)))  # (the filter dropped the others)
    ids, am, lab = want["input_ids"], want["attention_mask"], want["labels"]
    only_close = ((ids[:, 0] == SEP) | (lab[:, 0] == SEP)) & ((am == 0).sum(axis=1) == 1)  # (l = 1; [SEP] may be masked)
    assert only_close.sum() >= 2, "no row that holds only the closing frame"


def test_more_rows_than_waves(torch, native_lib):  # noqa: F811
    """S = 8 over 2.5 MB: more than 65,536 rows, so every wave of the capped grid writes several."""
    rng = np.random.default_rng(5)
    texts = [" ".join(FILLER[int(x)] for x in rng.integers(0, len(FILLER), int(rng.integers(200, 3000))))
             for _ in range(450)]
    size = sum(len(t) for t in texts)
    assert 2_000_000 < size < 3_000_000
    S, B = 8, 64
    want = oracle_lib.oracle_rows(oracle_lib.Tok(), texts, S, mask_length_of(S), 103, seed=SEED, B=B,
                                  first_record=FIRST)
    G = want.shape[1]
    assert G > 65536 and G % B != 0
    db = DeviceBatcher(batch_size=B, sequence_length=S, mask_length=mask_length_of(S), seed=SEED)
    res = run_device(torch, db, texts, first_record=FIRST)
    assert res.rows() == G
    Gp = -(-G // B) * B
    got = res.planes(Gp)
    for j in range(4):
        bad = np.nonzero((got[j][:G] != want[j]).any(axis=1))[0]
        assert bad.size == 0, f"plane {j}: {bad.size} of {G} rows differ, first {bad[:5]}"
    ids, am, tt, lab = got
    assert (ids[G:] == 0).all() and (am[G:] == 1).all() and (tt[G:] == 0).all() and (lab[G:] == -100).all()
    db.close()


@pytest.mark.parametrize("segments", [2, 3])
@pytest.mark.parametrize("S", [256, 512])
def test_pipelined_segments(torch, native_lib, S, segments, monkeypatch):  # noqa: F811
    """SegSel ranges other than the whole call reach the lean kernels."""
    monkeypatch.setenv("SDL_SEGMENTS", str(segments))
    monkeypatch.setenv("SDL_SEG_MIN_CHUNKS", "16")
    blobs = form_blobs(S, True)
    assert n_chunks(blobs) >= 16 * segments
    check(torch, "mlm", S, blobs, min_ids=MIN_IDS)
    check(torch, "multi-label", S, blobs_for("bert", True))


# ---- the calls that keep k_rows at these widths ------------------------------------------------------
@pytest.mark.parametrize("task", ["mlm", "clm"])
@pytest.mark.parametrize("S", [8, 256])
def test_per_record_pushes(native_lib, S, task):
    """Record by record into the host batches (row_one's direct destination), and the same
    records in one call."""
    blobs = blobs_for(TASK[task][2], False)
    B = partial_batch_size(sum(w["rows"] for w in oracle_batches(oracle_batcher(task, 3, S, min_ids=64), task, blobs)),
                           (3, 5, 7))
    want = oracle_batches(oracle_batcher(task, B, S, min_ids=64), task, blobs)
    assert len(want) > 2 and sum(w["rows"] for w in want) % B != 0
    one = host_batcher(task, B, S)
    per = drain(one, [d for d in (one.create_sync_batch(b) for b in blobs) if d is not None])
    assert_batches(task, S, per, want)
    many = host_batcher(task, B, S)
    bulk = drain(many, many.create_sync_batches(list(blobs)))
    assert_batches(task, S, bulk, want)
    one.close()
    many.close()


@pytest.mark.parametrize("lists", [False, True])
def test_rand_mode_rows(torch, native_lib, lists):  # noqa: F811
    """rng_mode 1 at S = 512: k_rows and its LATE pass, as before."""
    check(torch, "mlm", 512, blobs_for("bert", lists), rng_mode=1)
