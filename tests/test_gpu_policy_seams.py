"""Whole-word units across the two seams of the policy's unit build, through the three kernels
that each hold a copy of it (rows_device.hpp row_policy_one, pair_mlm.hip, pack_mlm.hip): the
unpaired rows, the pair-mlm rows and the packed mlm rows.  S = 260: MR = 2 rounds of 256 positions,
the second one mostly empty.

A word of four pieces lies on columns 254-257 of a row -- the round seam: whether column 256
continues a unit is lane 63's last candidate bit of the round before (x63), and the unit's start
reaches round 1 through the scan's carry.  A word of two pieces lies on columns 3-4 -- the lane
seam: lane 1's first element looks at lane 0's last (wave_prev).  The packed stream also lays a
word of four pieces across every row end, so that the next row begins inside a word: column 0 has
no position before it and starts a unit there.

All planes are compared exactly with the numpy models (mlm_policy_model.py, pair_mlm_model.py,
pack_mlm_model.py).  Each test first asserts on the model's output that the seam word is picked
whole in one row and left alone in another, so it cannot pass without the seam deciding something.
"""
import numpy as np
import pytest

import mlm_policy_model as M
import pack_mlm_model
import pack_model
import pair_mlm_model
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_pack_mlm import check, five, run as run_packed
from test_gpu_pair_mlm import assert_call, run_pairs, wp_ids
from test_gpu_parity import run_device, torch  # noqa: F401

pytestmark = pytest.mark.gpu

S, BSZ, POLICY = 260, 4, 2
MASK_LENGTH = 39  # int(0.15 S); per mille 150 gives the same budget for a full row
ROUND_SEAM, LANE_SEAM = (254, 255, 256, 257), (3, 4)
WORD4, WORD2, FILL = "zqxj", "qzv", "the"  # 4, 2 and 1 pieces in the proxy vocabulary (asserted)

# Found on the CPU: for seed = 1, 2, ... the model's planes of each test's own text were computed
# (mlm_policy_model.apply over unmasked_rows; pair_mlm_model.rows; pack_mlm_model.pack) and the
# first seed taken at which assert_seams_decide holds -- the round-seam word picked in one row and
# not in another, the lane-seam word likewise -- and, packed, the half word at the head of a row
# is picked in one row and not in another.
SEED_ROWS, SEED_PAIRS, SEED_PACKED = 2, 2, 3


def words_at(n_ids, placed):
    """Words whose ids number n_ids, with `placed` {id index: word} and FILL elsewhere."""
    pieces = {WORD4: 4, WORD2: 2}
    out, i = [], 0
    while i < n_ids:
        w = placed.get(i, FILL)
        out.append(w)
        i += pieces.get(w, 1)
    assert i == n_ids
    return out


def assert_seams_decide(planes, rows, what):
    """On the model's planes: each seam word is picked whole in some row and not at all in another
    (a word is a unit: never picked in part)."""
    labels = planes[3]
    for cols in (ROUND_SEAM, LANE_SEAM):
        picked = [(labels[g, list(cols)] != -100) for g in rows]
        assert all(p.all() or not p.any() for p in picked), (what, cols)
        assert any(p.all() for p in picked) and any(not p.any() for p in picked), (what, cols)


@pytest.fixture(scope="module")
def pieces(oracle_tok):
    _, cont, _, _ = M.proxy_vocab()
    w4, w2, w1 = (wp_ids(oracle_tok, w) for w in (WORD4, WORD2, FILL))
    assert (len(w4), len(w2), len(w1)) == (4, 2, 1)
    assert [bool(cont[i]) for i in w4 + w2 + w1] == [False, True, True, True, False, True, False]
    return w4, w2


def test_unpaired_rows(torch, native_lib, pieces):  # noqa: F811
    # a record's rows: [CLS] [CLS] ids [SEP] [SEP] [SEP] cut to S, so id i lies on column 2 + i of
    # chunk 0 and the last closing id makes a chunk 1 of one position
    n = 6
    texts = [" ".join(words_at(256, {1: WORD2, 252: WORD4}))] * n
    rows, where = M.unmasked_rows(texts, S, min_ids=0)
    assert where == [(r, c, l) for r in range(n) for c, l in ((0, S), (1, 1))]
    w4, w2 = pieces
    seam_rows = range(0, 2 * n, 2)
    for g in seam_rows:
        assert rows[0, g, list(ROUND_SEAM)].tolist() == w4 and rows[0, g, list(LANE_SEAM)].tolist() == w2
    want, _ = M.apply(rows, where, POLICY, SEED_ROWS, MASK_LENGTH)
    assert_seams_decide(want, seam_rows, "unpaired")
    db = DeviceBatcher(batch_size=BSZ, sequence_length=S, seed=SEED_ROWS, min_ids=0, mask_policy=POLICY,
                       mask_per_mille=150, mask_length=MASK_LENGTH)
    res = run_device(torch, db, texts)
    assert res.rows() == 2 * n
    got = np.stack(res.planes(2 * n))
    for p, name in enumerate(("input_ids", "attention_mask", "token_type_ids", "labels")):
        np.testing.assert_array_equal(got[p], want[p], err_msg=name)
    db.close()


def test_pair_mlm_rows(torch, native_lib, pieces, oracle_tok):  # noqa: F811
    # [CLS] at 0, A on columns 1..100, [SEP] at 101, B on columns 102..257, [SEP] at 258
    a = " ".join(words_at(100, {2: WORD2}))
    b = " ".join(words_at(156, {152: WORD4}))
    pairs = [(a, b)] * 6
    ids = [(wp_ids(oracle_tok, a), wp_ids(oracle_tok, b))] * 6
    want = pair_mlm_model.rows(ids, S, native.SDL_PAIR_MLM, POLICY, SEED_PAIRS, 0, MASK_LENGTH, 150, B=BSZ)
    w4, w2 = pieces
    plain, _, fill = pair_mlm_model.unmasked(ids, S, native.SDL_PAIR_MLM, SEED_PAIRS)
    assert fill == [259] * 6
    assert plain[0, 0, list(ROUND_SEAM)].tolist() == w4 and plain[0, 0, list(LANE_SEAM)].tolist() == w2
    assert_seams_decide(want["planes"], range(6), "pairs")
    db = DeviceBatcher(task=native.SDL_TASK_MLM, batch_size=BSZ, sequence_length=S, pair=native.SDL_PAIR_MLM,
                       mask_policy=POLICY, mask_per_mille=150, seed=SEED_PAIRS, mask_length=MASK_LENGTH)
    res, _ = run_pairs(torch, db, pairs)
    assert_call(res, want, 6, BSZ)
    db.close()


def test_packed_rows_and_flush(torch, native_lib, pieces, oracle_tok):  # noqa: F811
    # one document: [CLS] at stream position 0, id i at position 1 + i; in every row the two seam
    # words, and a word of four pieces on the row's last two columns and the next row's first two
    rows_n, tail = 5, 40
    placed = {}
    for g in range(rows_n):
        placed[g * S + 3 - 1] = WORD2
        placed[g * S + 254 - 1] = WORD4
        placed[g * S + 258 - 1] = WORD4
    text = " ".join(words_at(rows_n * S + tail - 1, placed))
    ids = [wp_ids(oracle_tok, text)]
    want, carry = pack_mlm_model.pack(ids, S, 0, pack_model.EMPTY, 0, POLICY, SEED_PACKED, MASK_LENGTH)
    w4, w2 = pieces
    _, cont, _, _ = M.proxy_vocab()
    assert want.shape[1] == rows_n and len(carry[0]) == tail + 1
    unmasked = np.where(want[3] != -100, want[3], want[0])
    for g in range(rows_n):
        assert unmasked[g, list(ROUND_SEAM)].tolist() == w4 and unmasked[g, list(LANE_SEAM)].tolist() == w2
    for g in range(1, rows_n):  # the row begins inside a word: its first two columns are a unit
        assert unmasked[g, :2].tolist() == w4[2:] and cont[unmasked[g, 0]]
        head = want[3, g, :2] != -100
        assert head.all() or not head.any()
    heads = [(want[3, g, :2] != -100).all() for g in range(1, rows_n)]
    assert any(heads) and not all(heads)
    assert_seams_decide(want, range(rows_n), "packed")
    db = DeviceBatcher(batch_size=BSZ, sequence_length=S, seed=SEED_PACKED, min_ids=0, mask_policy=POLICY, pack=1,
                       mask_per_mille=150, mask_length=MASK_LENGTH)
    res = run_packed(torch, db, [text])
    assert res.rows() == rows_n
    check(five(res), want, "packed")
    fl = db.flush_device()
    torch.cuda.synchronize()
    wf = pack_mlm_model.flush(carry, S, rows_n, POLICY, SEED_PACKED, MASK_LENGTH)
    assert fl.rows() == 1 and cont[carry[0][0]]  # (the flush row begins inside a word as well)
    check(five(fl), wf, "flush")
    db.close()
