"""GPU parity of the rows kernel reading the WordPiece chunk lists themselves (pipeline.hip
k_rows<.., LISTS>, rows_device.hpp row_one, list_index.hpp): on the large WordPiece path (more
than SMALL_CHUNKS = 64 chunks) no dense id array is made, each row finds its first chunk
(k_row_map) and its ids' chunks from one load of chunk boundaries, or -- rows over long runs of
chunks without ids -- by a search per lane.

Every arena is 100-400 KiB (a few hundred rows) and every row of every plane is compared
bit-exactly with the CPU oracle; nothing is sampled."""
import functools
import random

import numpy as np
import pytest

import oracle_lib
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher, arena_from_texts

from test_gpu_parity import run_device, torch  # noqa: F401
from test_gpu_wordpiece_groups import ACCENTED, LETTERS, odd_word

pytestmark = pytest.mark.gpu

CHUNK = 1024
FILLER = "the of and to in a is that for it as was with be by on not he".split()


def words(rng, n):
    return " ".join(rng.choice(FILLER) for _ in range(n))


def arena_bytes(texts):
    return sum(len(t.encode("utf-8")) for t in texts)


def assert_large_path(texts):
    n = arena_bytes(texts)
    assert 100 << 10 <= n <= 400 << 10, n
    assert -(-n // CHUNK) > 64


# ---- the arenas (built once; the oracle's rows once per arena and shape) -----------------
@functools.lru_cache(maxsize=None)
def empty_chunk_texts():
    """Runs of spaces / newlines of 3, 70 and 130 KiB between words -- rows over 3, more than
    64 and more than 128 chunks without ids -- and runs at a record's start and at its end."""
    rng = random.Random(11)
    texts = []
    for gap in (3 << 10, 70 << 10, 130 << 10):
        ws = "".join(rng.choice(" \n") for _ in range(gap))
        texts.append(words(rng, 90) + ws + words(rng, 300) + " " + ws[:2500] + words(rng, 200))
        texts.append(words(rng, 120))
    texts.append(" " * 5000 + words(rng, 700))  # a run at the record's start ...
    texts.append(words(rng, 700) + "\n" * 5000)  # ... and at its end
    texts.append(" \n" * 2000 + words(rng, 80) + " " * 9000 + words(rng, 80) + "\n " * 2000)
    for _ in range(10):  # 3-5 KiB runs at other places of a row
        ws = "".join(rng.choice(" \n\t\r") for _ in range(rng.randint(3 << 10, 5 << 10)))
        texts.append(words(rng, rng.randint(1, 500)) + ws + words(rng, rng.randint(100, 600)))
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def dense_texts():
    """1,024 ids a chunk ('!' runs) and one id every two bytes ('a ' runs): every row crosses
    list boundaries, at every 2-byte alignment of the lists."""
    rng = random.Random(12)
    texts = []
    while arena_bytes(texts) < 150 << 10:
        texts.append("!" * rng.randint(3000, 5000))
        texts.append("a " * rng.randint(700, 2600) + ("a" if rng.random() < 0.5 else ""))
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def coincidence_texts(S):
    """Records that start exactly at a chunk boundary (every record is a whole number of chunks:
    '!' for ids, spaces to the chunk's end) whose first chunk holds S - 1 ids and whose middle
    chunks hold S, so with the one [CLS] every row begins at a list's first id and ends at its
    last; the last chunk's count makes the framed length 0, 1, S-3, S-2, S-1 (mod S)."""
    assert S <= CHUNK
    def chunk_of(n_ids):
        return "!" * n_ids + " " * (CHUNK - n_ids)
    texts = []
    for rep in range(5):
        for want in (0, 1, S - 3, S - 2, S - 1):
            last = (want - 2) % S  # framed = (S - 1) + S * mid + last + 3
            if last == 0:
                last = S
            mid = 3 + rep
            t = chunk_of(S - 1) + chunk_of(S) * mid + chunk_of(last)
            assert (S - 1 + S * mid + last + 3) % S == want
            texts.append(t)
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def filter_texts():
    """Zero-length records and records under the 64-id filter between long ones, first and last
    included."""
    rng = random.Random(14)
    texts = ["", words(rng, 20)]
    while arena_bytes(texts) < 130 << 10:
        texts += [words(rng, rng.randint(400, 1500)), "", words(rng, rng.randint(1, 59)), "", "",
                  "!" * rng.randint(1, 60), words(rng, rng.randint(61, 70))]
    texts += [words(rng, 30), ""]
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def heldout_texts():
    """Chunks with 1-40 multi-id words (test_gpu_wordpiece_groups' generator) among filler, plus
    words of 17-100 chars (the deferred lattice), words of more than 100 chars ([UNK]), accented
    words, and -- placed by byte offset -- a long word that starts in a chunk's last 16 bytes and
    runs 100 bytes into the next, with record boundaries directly before and after such words."""
    rng = random.Random(18)
    texts, pos = [], 0  # pos: arena bytes so far

    def push(t):
        nonlocal pos
        texts.append(t)
        pos += len(t.encode("utf-8"))

    def long_word(n):
        return "".join(rng.choice(LETTERS) for _ in range(n))

    multi = [1, 2, 3, 5, 8, 9, 13, 16, 17, 21, 27, 33, 40]
    while pos < 200 << 10:
        pending = rng.choice(multi)
        ws = [odd_word(rng, rng.random() < 0.3) for _ in range(pending)]
        ws += [rng.choice(FILLER) for _ in range(max(0, 150 - pending))]
        ws += [long_word(rng.randint(17, 100)) for _ in range(rng.randint(0, 3))]
        if rng.random() < 0.3:
            ws.append(long_word(rng.randint(101, 160)))
        if rng.random() < 0.3:
            ws.append("".join(rng.choice(ACCENTED + LETTERS) for _ in range(rng.randint(17, 40))))
        rng.shuffle(ws)
        push(" ".join(ws))
        # a word from the chunk's last 16 bytes to 100 bytes into the next chunk: pad this record
        # with filler up to the start byte; the word ends the record, begins the next one, or both
        start_in = CHUNK - rng.randint(1, 16)
        n_head = (start_in - pos) % CHUNK + CHUNK
        head = words(rng, 1000)[:n_head - 1] + " "  # (ASCII: bytes = chars)
        assert (pos + len(head)) % CHUNK == start_in
        w = long_word(CHUNK - start_in + 100)
        kind = rng.randrange(3)
        if kind == 0:    # ... | head word | next
            push(head + w)
        elif kind == 1:  # ... head | word tail
            push(head)
            push(w + " " + words(rng, 100))
        else:            # ... head | word | tail
            push(head)
            push(w)
            push(words(rng, 100))
    return tuple(texts)


@functools.lru_cache(maxsize=None)
def mlm_want(name, S, B, first_record, seed):
    texts = ARENAS[name]() if name in ARENAS else coincidence_texts(S)
    want = oracle_lib.oracle_rows(oracle_lib.Tok(), list(texts), S, int(np.float32(S) * np.float32(0.15)), 103,
                                  seed=seed, B=B, first_record=first_record)
    want.setflags(write=False)
    return want


ARENAS = {"empty": empty_chunk_texts, "dense": dense_texts, "filter": filter_texts, "heldout": heldout_texts}


def check_mlm(torch, name, S=512, B=32, first_record=0, seed=7):  # noqa: F811
    """Masks on (the default mask_length): all four planes of every row, padding rows included."""
    texts = list(ARENAS[name]() if name in ARENAS else coincidence_texts(S))
    assert_large_path(texts)
    want = mlm_want(name, S, B, first_record, seed)
    db = DeviceBatcher(batch_size=B, sequence_length=S, seed=seed)
    res = run_device(torch, db, texts, first_record=first_record)
    G = res.rows()
    assert want.shape[1] == G and G > 0
    Gp = -(-G // B) * B
    got = res.planes(Gp)
    for j in range(4):
        bad = np.nonzero((got[j][:G] != want[j]).any(axis=1))[0]
        assert bad.size == 0, f"{name} S={S}: plane {j}, {bad.size} of {G} rows differ, first {bad[:5]}"
    ids, am, tt, lab = got
    assert (ids[G:] == 0).all() and (am[G:] == 1).all() and (tt[G:] == 0).all() and (lab[G:] == -100).all()
    assert int(res.record_rows().sum()) == G
    db.close()
    return G, Gp


def test_empty_chunks_inside_rows(torch, native_lib):  # noqa: F811
    check_mlm(torch, "empty")


def test_dense_chunks(torch, native_lib):  # noqa: F811
    check_mlm(torch, "dense")


def test_rows_begin_and_end_on_list_boundaries(torch, native_lib):  # noqa: F811
    check_mlm(torch, "coincidence", S=512)


def test_filtered_and_empty_records(torch, native_lib):  # noqa: F811
    check_mlm(torch, "filter")


@pytest.mark.parametrize("name", ["empty", "dense", "coincidence"])
@pytest.mark.parametrize("S", [128, 1024, 100])
def test_shapes(torch, native_lib, name, S):  # noqa: F811
    """MR 1, MR 4 and the scalar store path (S not a multiple of 4); a last batch that needs
    padding rows; a non-zero first_record."""
    G, Gp = check_mlm(torch, name, S=S, B=24, first_record=1000003)
    assert Gp >= G


def test_last_batch_needs_padding(torch, native_lib):  # noqa: F811
    G, Gp = check_mlm(torch, "filter", S=512, B=37, first_record=5)
    assert Gp > G


def test_single_class_over_a_large_arena(torch, native_lib, oracle_tok):  # noqa: F811
    rng = random.Random(16)
    texts = list(empty_chunk_texts()[:2]) + [words(rng, rng.choice([0, 3, 90, 400, 900])) for _ in range(220)]
    texts += ["!" * 4000, " " * 3000, ""]
    assert_large_path(texts)
    labels = [rng.randrange(2) for _ in texts]
    S, Bsz = 128, 32
    arena, offs = arena_from_texts(texts)
    ta = torch.from_numpy(np.concatenate([arena, np.zeros(16, np.uint8)])).cuda()
    to = torch.from_numpy(offs.astype(np.int64)).cuda()
    tl = torch.tensor(labels, dtype=torch.int32).cuda()
    tlo = torch.arange(len(texts) + 1, dtype=torch.int64).cuda()
    db = DeviceBatcher(task=native.SDL_TASK_SINGLE_CLASS, batch_size=Bsz, sequence_length=S)
    res = db.process_labels(ta.data_ptr(), arena.size, to.data_ptr(), len(texts), tl.data_ptr(), tlo.data_ptr())
    torch.cuda.synchronize()
    assert res.rows() == len(texts) and res.label_errors() == 0
    ids, am, tt, lab = res.planes()
    ob = oracle_lib.OracleBatcherEx(oracle_lib.Encoder("bert", oracle_tok), oracle_lib.SINGLE_CLASS, Bsz, S)
    want = [r for r in (ob.push(t, [l]) for t, l in zip(texts, labels)) if r is not None]
    want.append(ob.flush())
    n = len(texts)
    np.testing.assert_array_equal(ids, np.concatenate([w["input_ids"] for w in want])[:n])
    np.testing.assert_array_equal(am, np.concatenate([w["attention_mask"] for w in want])[:n])
    np.testing.assert_array_equal(tt, np.zeros_like(tt))
    np.testing.assert_array_equal(lab[:, 0], labels)
    db.close()


@pytest.mark.parametrize("name", ["empty", "dense"])
def test_pipelined_segments(torch, native_lib, name, monkeypatch):  # noqa: F811
    """Segment k's rows read only the lists and offsets of chunks the tokenizer launches <= k wrote."""
    monkeypatch.setenv("SDL_SEGMENTS", "3")
    monkeypatch.setenv("SDL_SEG_MIN_CHUNKS", "16")
    check_mlm(torch, name)


def test_heldout_style_chunks(torch, native_lib):  # noqa: F811
    """Multi-id words, deferred-lattice words, [UNK] words and words that run past their chunk's
    end (the [CHUNK, STAGE) stage slots), with record boundaries right before and after them
    (rec_local)."""
    check_mlm(torch, "heldout")
