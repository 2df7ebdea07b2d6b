"""GPU parity at the shapes where the glue kernels between the tokenizer and the rows take another
path (pipeline.hip): the two-launch scans (k_scan_reduce, k_scan_apply: more than 8,192 chunks),
the row scan fused with the row map over k_records_tiles' sums (k_scan_rows_map: more than 8,192
records, and more than 262,144, where a block takes several tiles), and k_chunk_ranges' searches
in the block's bracket of offsets (a bracket longer than its LDS cap, a record over several
blocks, empty records at a block's edge).

Every row of every plane is compared with the CPU oracle's; nothing is sampled."""
import random

import numpy as np
import pytest

import oracle_lib
from streaming_data_loader_amd.device import DeviceBatcher

from test_gpu_parity import run_device, torch  # noqa: F401

pytestmark = pytest.mark.gpu

CHUNK = 1024
BLOCK = 256 * CHUNK  # the bytes of a k_chunk_ranges block's chunks
FILLER = "the of and to in a is that for it as was with be by on not he".split()
SHORT = ["", "a", "ab cd ef g", "of the and", "!", "it was not"]  # under the 64-id filter: no rows


def words(rng, n):
    return " ".join(rng.choice(FILLER) for _ in range(n))


def text_of(rng, nbytes):
    """ASCII filler of exactly nbytes bytes."""
    t = words(rng, nbytes // 3 + 2)[:nbytes]
    assert len(t) == nbytes
    return t


def check(torch, texts, S, B, seed=7, first_record=3):  # noqa: F811
    k = int(np.float32(S) * np.float32(0.15))
    want = oracle_lib.oracle_rows(oracle_lib.Tok(), texts, S, k, 103, seed=seed, B=B, first_record=first_record)
    db = DeviceBatcher(batch_size=B, sequence_length=S, seed=seed)
    res = run_device(torch, db, texts, first_record=first_record)
    G = res.rows()
    assert want.shape[1] == G and G > 0, (want.shape, G)
    Gp = -(-G // B) * B
    got = res.planes(Gp)
    for j in range(4):
        bad = np.nonzero((got[j][:G] != want[j]).any(axis=1))[0]
        assert bad.size == 0, f"plane {j}: {bad.size} of {G} rows differ, first {bad[:5]}"
    ids, am, tt, lab = got
    assert (ids[G:] == 0).all() and (am[G:] == 1).all() and (tt[G:] == 0).all() and (lab[G:] == -100).all()
    rr = res.record_rows()
    assert int(rr.sum()) == G
    db.close()
    return rr


@pytest.mark.parametrize("R", [8193, 16383, 16384, 16385, 262144 + 257])
def test_many_short_records_among_long_ones(torch, native_lib, R):  # noqa: F811
    """Records the filter drops (no rows) among records of several rows: the rows of one tile of
    256 records are few and unevenly spread, records with rows sit at the tiles' first and last
    places, and the last tile is partial.  Past 262,144 records k_records' grid is capped (a block
    takes more than one tile) and so is the scan's."""
    rng = random.Random(R)
    S, B = 128, 8
    every = 40 if R < 100000 else 400
    texts = []
    for r in range(R):
        edge = r % 256 in (0, 255) and (r // 256) % 3 == 0
        if edge or rng.randrange(every) == 0 or r >= R - 2:
            texts.append(words(rng, rng.choice([70, 130, 260, 400, 700])))  # 1 to 6 rows
        else:
            texts.append(SHORT[rng.randrange(len(SHORT))])
    rr = check(torch, texts, S, B)
    assert (rr == 0).sum() > R * 0.9 and (rr > 1).sum() > 50 and rr[-1] > 0 and rr[0] > 0


@pytest.mark.parametrize("n_chunks", [8193, 10240, 10241])
def test_many_chunks_of_ordinary_records(torch, native_lib, records, n_chunks):  # noqa: F811
    """More than 8,192 chunks: the chunk scan's tiles, a last tile of one chunk (8,193), exactly
    five tiles (10,240) and one chunk past them (10,241)."""
    rng = random.Random(n_chunks)
    want_bytes = (n_chunks - 1) * CHUNK + (CHUNK if n_chunks == 10240 else 1)
    texts, n = [], 0
    while True:
        t = records[rng.randrange(len(records))]
        b = len(t.encode("utf-8"))
        if n + b > want_bytes - 4096:
            break
        texts.append(t)
        n += b
    texts.append(text_of(rng, want_bytes - n))
    assert sum(len(t.encode("utf-8")) for t in texts) == want_bytes and -(-want_bytes // CHUNK) == n_chunks
    check(torch, texts, 512, 32)


def test_bracket_longer_than_the_lds_cap(torch, native_lib, records):  # noqa: F811
    """More than 2,048 one-byte and empty records inside the first block's 256 KiB (its bracket
    does not fit: the search of the whole offset array), ordinary text behind them and in the
    following blocks (brackets that fit)."""
    rng = random.Random(5)
    texts = [words(rng, 300)]
    texts += ["a" if i % 3 else "" for i in range(3000)]
    n = sum(len(t) for t in texts)
    assert n < BLOCK // 2
    while n < 3 * BLOCK + 5000:
        t = records[rng.randrange(len(records))]
        texts.append(t)
        n += len(t.encode("utf-8"))
    check(torch, texts, 128, 8)


def test_one_record_over_several_blocks(torch, native_lib, records):  # noqa: F811
    """A record of 2.6 blocks: the blocks inside it have a bracket of no offset or one."""
    rng = random.Random(6)
    texts = list(records[:20]) + [text_of(rng, 2 * BLOCK + 150000)] + list(records[20:40])
    check(torch, texts, 512, 8)


def test_empty_records_at_a_block_edge(torch, native_lib, records):  # noqa: F811
    """Empty records exactly at a block's first byte, a byte before it and a byte after it, and
    at the left edge of the block's first window."""
    rng = random.Random(8)
    texts, n = [], 0

    def fill_to(target):
        nonlocal n
        while target - n > 6000:
            t = text_of(rng, rng.randrange(300, 4000))
            texts.append(t)
            n += len(t)
        texts.append(text_of(rng, target - n))
        n = target

    fill_to(BLOCK - 1)
    texts += ["", ""]
    fill_to(BLOCK)  # (a one-byte record up to the edge)
    texts += ["", "", ""]
    fill_to(BLOCK + 1)
    texts += [""]
    fill_to(2 * BLOCK - 64)
    texts += ["", ""]
    fill_to(2 * BLOCK)
    texts += [""] * 5
    fill_to(2 * BLOCK + 70000)
    texts += ["", ""]
    assert sum(len(t) for t in texts) == n
    check(torch, texts, 128, 8)
