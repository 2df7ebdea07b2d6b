"""GPU parity for every merge path of the GPT-2 byte-level BPE tokenizer, on synthetic merge tables.

streaming_data_loader_amd/csrc/tokenize_bpe.hip settles a pre-token on one of six paths -- the word
table (17..64 bytes: tail compared with `vpool`), bpe_lane (misses of 2..LANE_BPE bytes),
bpe_wave_seg (LANE_BPE+1..BPE_MAX_WAVE bytes, several words packed into one wave), k_bpe_long in
LDS (..LONG_LDS symbols) and on the global scratch (longer), and pieces that run past their chunk's
window (len == 0, bpe_piece_end) -- and two more pieces of code depend on them: the rec_local /
chunk_cnt fix-up for records after a long piece, and the unpacked copy-out of a chunk with more
than 2 * WIN / 4 list entries.  On the proxy gpt2 vocabulary the long inputs of the other tests
merge in one or two rounds; the tables of tests/golden/make_bpe_merge_vocab.py make random words
merge over 10..50 rounds into as many distinct ids, with self-pairs (x, x) and (xy, xy) in the
middle of the ranks, so a wrong compaction offset, a stale cached pair value, a wrong `blocked`
hand-over between tiles or a wrong per-word minimum changes the ids.

Every case (CASES; one test per case and table seed)
  * builds its arenas and asserts its census condition while doing so (tests/bpe_census.py: the
    chunk kernel's classification of the input restated on the host, its limits read from the
    kernel sources), so the case says which side of which limit its input is on;
  * then compares every record's ids with the CPU oracle (oracle/orc_bpe.c), which
    tests/test_bpe_merge_vocab.py pins to `tokenizers` and to two plain models on the same tables;
  * asserts the device reported no tokenize error (d_tokenize_errors, k_bpe_long's list overflow).
Records are a whole number of 1,024-byte chunks where a case is about a chunk.  Ids per record come
from CLM rows (min_ids=0, S=2048) as test_gpu_gpt2.device_ids reads them; one DeviceBatcher per
table, arenas of <= 64 KiB.  Inputs are letter-words joined by single spaces: the letters a b c é
中 of the merge alphabet, and x y z outside it (one id a byte, no merge ever).
test_every_path_is_reached counts the pieces per path over all cases and prints them.

Not reached, and why:
  * a packed word's head next to lane 63: a wave-path word has > LANE_BPE symbols, so the highest
    head an input can give is lane 64 - (LANE_BPE + 1) = 51, and heads only move left afterwards;
    wave_head_high uses 51;
  * a known-length piece on the global form is only 1025..1047 bytes at chunk offsets 0..22 (any
    longer piece ends outside its chunk's window and arrives with len == 0); global_lengths has one;
  * the tail compare's retry after a header match in *both* slots; table_reject reaches the
    compare's reject side through strings whose hash names a token's slot -- one string for each
    of the token's two slots, so the occupied one is met -- assuming the word table of these
    ~400-entry vocabularies has at most 2^COLLIDE_BITS slots (it has 2^11);
  * the error flag's set side: the long-piece list holds N / 64 + n_chunks + 1 entries and a chunk
    lists at most CHUNK / 65 + 1 pieces, so no input overflows it; pinned is only that the flag
    is handed out and reads 0 after every call (neither a null pointer nor uninitialised memory).
"""
import random
import zlib

import numpy as np
import pytest

import bpe_census
import make_bpe_merge_vocab as mv
import make_t5_long_piece_vocab as lp
import oracle_lib
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher
from test_gpu_gpt2 import run, torch  # noqa: F401  (the module-scoped torch fixture)

pytestmark = pytest.mark.gpu
S = 2048
ARENA_MAX = 64 << 10
K = bpe_census.constants()
CH, LANE, WAVE, LDS, HR = K["CHUNK"], K["LANE_BPE"], K["BPE_MAX_WAVE"], K["LONG_LDS"], K["HALO_R"]
PACKED = 2 * K["WIN"] // 4  # list entries the packed copy-out holds
COLLIDE_BITS = 14
OUT = [b"x", b"y", b"z"]    # letters outside the merge alphabet


class Dev:
    """One table: its DeviceBatcher, oracle tokenizer, census and word material."""

    def __init__(self, seed, path):
        self.seed = seed
        self.t = mv.table(seed)
        self.tok = oracle_lib.Gpt2Tok(path)
        self.census = bpe_census.Census(self.t.is_self, self.t.encode_word)
        self.db = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=64, sequence_length=S, min_ids=0,
                                tokenizer=path)
        self.x = self.t.merges[mv.SELF1][0]    # (x, x) is a merge
        self.xy = self.t.merges[mv.SELF2][0]   # (xy, xy) is a merge
        spaced = sorted((s for s in self.t.ids if s[:1] == b" " and len(s) > 1 and s.isascii() and self.t.is_self(s)),
                        key=len)
        self.fill = spaced[0]                  # the filler word: a word-table hit
        self.long_self = self.t.self_encoding()
        self.built = {}

    def rng(self, name):
        return random.Random(zlib.crc32(name.encode()) + self.seed)

    def word(self, rng, n, letters=mv.LETTERS):
        return mv.random_word(rng, n, letters)

    def piece(self, rng, n, letters=mv.LETTERS):
        """A space and a random word, n bytes together, that is no word-table entry."""
        for _ in range(50):
            p = b" " + self.word(rng, n - 1, letters)
            if not self.t.is_self(p):
                return p
        return b" " + self.word(rng, n - 1, OUT)

    def pad(self, n, start=False):
        """Exactly n bytes of filler words (`start`: at a record's start, else after a word)."""
        if n == 0:
            return b""
        s = b"a" if start else b""
        while len(s) + len(self.fill) <= n:
            s += self.fill
        r = n - len(s)
        if r and not s:
            assert r >= 2, "one byte after a word cannot be a word"
            return b" " + b"x" * (r - 1)
        return s + b"x" * r

    def finish(self, body):
        """The record padded to a whole number of chunks."""
        r = -len(body) % CH
        return body + (b" " if r == 1 else self.pad(r, start=not body))

    def at(self, pos, piece, tail=b""):
        """A record of whole chunks with `piece` (its space first) at byte `pos`, then `tail`."""
        return self.finish(self.pad(pos, start=True) + piece + tail)

    def cen(self, blobs):
        offs = np.zeros(len(blobs) + 1, np.uint64)
        np.cumsum([len(b) for b in blobs], out=offs[1:])
        assert int(offs[-1]) <= ARENA_MAX
        return self.census.chunks(np.frombuffer(b"".join(blobs), np.uint8), offs)

    def check(self, torch, blobs):
        res = run(torch, self.db, blobs)
        assert res.tokenize_errors() == 0
        ids, am, _, _ = res.planes()
        per = res.record_rows()
        g = 0
        for r, b in enumerate(blobs):
            seq = []
            for _ in range(int(per[r])):
                z = int((am[g] == 0).sum())
                seq += ids[g, :S if z == 0 else z].tolist()
                g += 1
            want = self.tok.encode(b)
            if seq[1:-1] != want:
                got = seq[1:-1]
                k = next((i for i, (a, c) in enumerate(zip(got, want)) if a != c), min(len(got), len(want)))
                raise AssertionError(f"record {r} ({len(b)} bytes, {bytes(b[:40])!r}...): {len(got)} ids, oracle "
                                     f"{len(want)}; first difference at id {k}: {got[k:k + 6]} != {want[k:k + 6]}")


def paths(chunk, want=None):
    ps = [p[2] for p in chunk["pieces"]]
    return ps if want is None else ps.count(want)


def piece_at(chunks, pos):
    """(length, path) of the piece starting at byte pos."""
    for p, n, path in chunks[pos // CH]["pieces"]:
        if p == pos:
            return n, path
    raise AssertionError(f"no piece starts at {pos}")


CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


# ---- bpe_lane ------------------------------------------------------------------------------------
@case
def lane_lengths(d):
    """2, 3, LANE_BPE - 1 and LANE_BPE bytes: bpe_lane; LANE_BPE + 1: the wave path."""
    rng = d.rng("lane_lengths")
    lens = [2, 3, LANE - 1, LANE, LANE + 1] * 8
    body, pos = b"a", []
    for n in lens:
        pos.append(len(body))
        body += d.piece(rng, n)
    c = d.cen([d.finish(body)])
    for p, n in zip(pos, lens):
        assert piece_at(c, p) == (n, "lane" if n <= LANE else "wave")
    return [[d.finish(body)]]


@case
def lane_second_pass(d):
    """More than 64 (and more than 128) lane misses in one chunk: the q0 loop's later passes."""
    rng = d.rng("lane_second_pass")
    body = b"a" + b"".join(d.piece(rng, 4) for _ in range(250))
    c = d.cen([d.finish(body)])
    assert len(c) == 1 and paths(c[0], "lane") > 2 * 64 and paths(c[0], "wave") == 0
    return [[d.finish(body)]]


@case
def lane_mixed_with_hits(d):
    """Hits and lane misses alternate: the pending list is sparse in the piece list."""
    rng = d.rng("lane_mixed")
    hits = [s for s in d.t.ids if s[:1] == b" " and 2 <= len(s) <= 16 and d.t.is_self(s)]
    body = b"a"
    while len(body) < CH - 40:
        body += rng.choice(hits) + d.piece(rng, rng.randint(2, LANE))
    c = d.cen([d.finish(body)])
    assert paths(c[0], "hit") >= 30 and paths(c[0], "lane") >= 30
    return [[d.finish(body)]]


@case
def lane_self_pair_runs(d):
    """Odd and even runs of the self-pair letter and token in words of <= LANE_BPE bytes: of equal
    ranks bpe_lane takes the leftmost."""
    rng = d.rng("lane_runs")
    body, n_runs = b"a", 0
    while len(body) < CH - 2 * LANE:
        base = rng.choice([d.x, d.x, d.xy])
        run = base * rng.randint(2, (LANE - 3) // len(base))
        w = b" " + rng.choice([b""] + OUT + mv.LETTERS[:3]) + run
        w += d.word(rng, rng.randint(0, LANE - len(w)), OUT + mv.LETTERS[:3])
        if not d.t.is_self(w):
            body += w
            n_runs += 1
    c = d.cen([d.finish(body)])
    assert paths(c[0], "lane") >= n_runs > 64 and paths(c[0], "wave") == 0
    return [[d.finish(body)]]


# ---- bpe_wave_seg ----------------------------------------------------------------------------------
def _packs(d, name, groups, letters=mv.LETTERS):
    """One chunk per group of piece lengths; the census must pack each chunk as `want` says."""
    rng = d.rng(name)
    blobs = []
    for lens, want in groups:
        body = b"a" + b"".join(d.piece(rng, n, letters) for n in lens)
        blobs.append(d.finish(body))
    c = d.cen(blobs)
    for ch, (lens, want) in zip(c, groups):
        assert ch["packs"] == want, (ch["packs"], want)
    return [blobs]


@case
def wave_single_words(d):
    """LANE_BPE + 1, + 2, 63 and 64 bytes (n == 64: every lane a symbol), one word a wave."""
    return _packs(d, "wave_single", [([n], [[n]]) for n in (LANE + 1, LANE + 2, WAVE - 1, WAVE)] +
                  [([WAVE, WAVE - 1, WAVE], [[WAVE], [WAVE - 1], [WAVE]])])


@case
def wave_exact_fill(d):
    """Packings that fill the 64 lanes exactly."""
    return _packs(d, "wave_exact", [([16] * 4, [[16] * 4]), ([32, 32], [[32, 32]]),
                                    ([16] * 8 + [32, 32], [[16] * 4, [16] * 4, [32, 32]])])


@case
def wave_break_at_limit(d):
    """Four words fit, the fifth starts the next packing; 52 + 13 breaks too."""
    return _packs(d, "wave_break", [([13] * 5, [[13] * 4, [13]]), ([52, 13, 51, 13], [[52], [13, 51], [13]])])


@case
def wave_skips_lane_words(d):
    """A LANE_BPE-byte miss between wave words is bpe_lane's: the packing loop steps over it."""
    g = [([52, LANE], [[52]]), ([40, LANE, 24], [[40, 24]]), ([LANE, 13, 3, 2, 13, LANE, 13, 13, 5, 13], [[13] * 4, [13]])]
    return _packs(d, "wave_skips", g)


@case
def wave_head_high(d):
    """The highest head an input can give: a 13-byte word at lanes 51..63 behind a 51-byte one."""
    return _packs(d, "wave_head_high", [([51, 13], [[51, 13]]), ([13, 13, 13, 25], [[13, 13, 13, 25]]),
                                        ([38, 13, 13], [[38, 13, 13]])])


@case
def wave_depth_mix(d):
    """Words of very different merge depth share a wave: one that collapses to two ids (a long
    vocabulary string and one letter outside the alphabet) beside one that does not merge at all,
    and beside a random one."""
    rng = d.rng("wave_depth")
    toks = [s for s in d.long_self if s[:1] != b" " and len(s) <= 30]
    blobs = []
    for i in range(6):
        t = rng.choice(toks)
        deep = b" " + t + b"x"
        flat = b" " + d.word(rng, 62 - len(deep), OUT)
        mid = d.piece(rng, WAVE - len(deep) - len(flat) + 14) if len(deep) + len(flat) <= 50 else b""
        order = [deep, flat] if i % 2 else [flat, deep]
        body = b"a" + b"".join(order) + mid
        blobs.append(d.finish(body))
        assert len(d.t.encode_word(deep)) <= 3 and len(d.t.encode_word(flat)) == len(flat)
    for ch in d.cen(blobs):
        assert len(ch["packs"][0]) >= 2 and sum(ch["packs"][0]) > 50
    return [blobs]


@case
def wave_self_pair_runs(d):
    """Odd and even runs of the self-pair letter and of the self-pair token inside packed words."""
    rng = d.rng("wave_runs")
    blobs = []
    for base in (d.x, d.xy):
        body = b"a"
        for n in range(2, 12):
            w = b" " + rng.choice(OUT + mv.LETTERS[:3]) + base * n + rng.choice(OUT) + base * (n + 1)
            body += w + d.word(rng, max(0, LANE + 1 - len(w)))
        blobs += [d.finish(body)]
    c = d.cen(blobs)
    assert all(paths(ch, "wave") >= 8 and any(len(p) > 1 for p in ch["packs"]) for ch in c)
    return [blobs]


# ---- k_bpe_long, LDS form ----------------------------------------------------------------------------
@case
def lds_lengths(d):
    """65, 66, 127, 128, 129 bytes in one chunk; 1023 and 1024 from a chunk's first byte."""
    rng = d.rng("lds_lengths")
    lens = [WAVE + 1, WAVE + 2, 127, 128, 129]
    body, pos = b"a", []
    for n in lens:
        pos.append(len(body))
        body += d.piece(rng, n)
    blobs = [d.finish(body)] + [d.finish(d.word(rng, n) + d.fill) for n in (LDS - 1, LDS)]
    c = d.cen(blobs)
    for p, n in zip(pos, lens):
        assert piece_at(c, p) == (n, "long_lds")
    assert piece_at(c, CH) == (LDS - 1, "long_lds") and piece_at(c, 3 * CH) == (LDS, "long_lds")
    return [blobs]


def _run_piece(pre, run, rng, d, tail=40):
    """`pre` letters outside the alphabet (they never merge, so the run keeps its symbol positions
    until its rank comes up), the run, one more such letter, a random tail."""
    return d.word(rng, pre, OUT) + run + rng.choice(OUT) + d.word(rng, tail)


@case
def lds_run_over_tile_edge(d):
    """A self-pair run over symbols 63 | 64: the merge that lands on a tile's last lane is
    carried into the next tile by `blocked`; every alignment, odd and even lengths."""
    rng = d.rng("lds_tile_edge")
    blobs = []
    for pre in range(58, 65):
        for n in (3, 4, 5, 6, 9):
            blobs.append(_run_piece(pre, d.x * n, rng, d))                    # each its own record
    for pre in range(59, 65):
        blobs.append(_run_piece(pre, d.xy * rng.randint(3, 8), rng, d))
    straddle = sum(1 for b in blobs[:35] if b[62:65] == d.x * 3)
    assert straddle >= 10  # symbols 62, 63 and 64 are all in the run
    for ch in d.cen(blobs):
        assert all(path in ("long_lds", "past") for _, _, path in ch["pieces"]) and set(ch["form"].values()) == {"lds"}
    return [blobs]


@case
def lds_run_over_two_tile_edges(d):
    """A self-pair run from before symbol 64 to past symbol 128."""
    rng = d.rng("lds_two_edges")
    blobs = []
    for pre in (59, 60, 61, 62, 63):
        for n in (70, 71):
            blobs.append(_run_piece(pre, d.x * n, rng, d))
        blobs.append(_run_piece(pre, d.xy * 40, rng, d))
    for b in blobs:
        assert WAVE + 1 < len(b) <= LDS and b[63:129] in (d.x * 66, (d.xy * 40)[:66], (d.xy * 40)[1:67])
    for ch in d.cen(blobs):
        assert set(ch["form"].values()) <= {"lds"} and "wave" not in paths(ch)
    return [blobs]


@case
def lds_shrinks_below_a_tile(d):
    """Pieces of 65..130 symbols that end as fewer than 64 (often fewer than 10) ids."""
    rng = d.rng("lds_shrinks")
    toks = [s for s in d.long_self if s[:1] != b" "]
    body, want = b"a", []
    for i in range(8):
        w = d.piece(rng, rng.randint(WAVE + 1, 130)) if i % 2 else b" " + b"".join(rng.sample(toks, 4))[:126]
        assert len(w) > WAVE and len(d.t.encode_word(w)) < WAVE
        want.append(len(body))
        body += w
    c = d.cen([d.finish(body)])
    assert all(piece_at(c, p)[1] == "long_lds" for p in want)
    return [[d.finish(body)]]


# ---- k_bpe_long, global form -------------------------------------------------------------------------
@case
def global_lengths(d):
    """1025 (from a chunk's first byte: the one known length past LONG_LDS), 1500 and 3000 bytes,
    aperiodic: each takes >= 10 merge rounds and ends as >= 10 distinct ids."""
    rng = d.rng("global_lengths")
    ws = [d.word(rng, n) for n in (LDS + 1, 1500, 3000, LDS + 2)]
    for w in ws:
        rounds, distinct = d.t.rounds(w)
        assert rounds >= mv.MIN_ROUNDS and distinct >= mv.MIN_DISTINCT
    blobs = [d.finish(w + d.fill) for w in ws]
    c = d.cen(blobs)
    assert piece_at(c, 0) == (LDS + 1, "long_global")
    assert piece_at(c, 2 * CH) == (1500, "past") and piece_at(c, 4 * CH) == (3000, "past")
    assert [f for ch in c for f in ch["form"].values()] == ["global"] * 4
    return [blobs]


@case
def global_piece_over_three_chunks(d):
    """A 2,100-byte piece from the middle of a chunk; records start in the chunk where it ends."""
    rng = d.rng("global_three")
    w = d.piece(rng, 2100)
    assert d.t.rounds(w)[0] >= mv.MIN_ROUNDS
    r0 = d.pad(500, start=True) + w
    end = len(r0)
    short = [d.word(rng, rng.randint(2, 30)) for _ in range(6)]
    blobs = [r0] + short
    blobs.append(d.finish(b"".join(blobs))[len(b"".join(blobs)):])
    c = d.cen(blobs)
    assert piece_at(c, 500) == (2100, "past") and c[0]["form"][500] == "global"
    assert end // CH == 2 and c[1]["pieces"] == [] and len(c[2]["pieces"]) > 6
    return [blobs]


# ---- the window's right edge ---------------------------------------------------------------------------
def _edge(d, name, start, end, path, form=None):
    """A piece from chunk offset `start` to `end` (chunk 0 of a two-chunk record)."""
    rng = d.rng(name)
    blobs = []
    for letters in (mv.LETTERS, OUT):
        blobs.append(d.at(start, d.piece(rng, end - start, letters), d.fill * 3))
    c = d.cen(blobs)
    for r in range(2):
        assert piece_at(c, 2 * r * CH + start) == (end - start, path)
        assert c[2 * r]["form"].get(2 * r * CH + start) == form and c[2 * r]["pieces"][-1][0] == 2 * r * CH + start
    return [blobs]


@case
def edge_last_end_the_window_shows(d):
    """From the chunk's last 10 bytes to c1 + HALO_R - 9: the last end the window shows."""
    return _edge(d, "edge_in", CH - 10, CH + HR - 9, "wave")


@case
def edge_first_end_past_the_window(d):
    """The same piece one byte longer: len == 0, bpe_piece_end finds its end."""
    return _edge(d, "edge_past", CH - 10, CH + HR - 8, "past", "lds")


@case
def edge_word_over_c1(d):
    """A 40-byte piece with c1 in its middle, and one that ends exactly at c1."""
    return [_edge(d, "edge_mid", CH - 20, CH + 20, "wave")[0] + _edge(d, "edge_at_c1", CH - 40, CH, "wave")[0]]


@case
def edge_short_piece_past_the_window(d):
    """Pieces of 30 and 200 bytes that start late in a chunk and end past its window: below and
    above BPE_MAX_WAVE, both len == 0."""
    return [_edge(d, "edge_30", CH - 4, CH + 26, "past", "lds")[0] + _edge(d, "edge_200", CH - 100, CH + 100, "past", "lds")[0]]


@case
def edge_text_end(d):
    """The last piece ends at the text end: in the chunk, in the next chunk's first bytes (the
    window shows the end of the text), and far beyond; wave, lane and long pieces."""
    rng = d.rng("edge_text_end")
    arenas = []
    for start, n in ((300, 20), (300, 5), (300, 200), (CH - 10, 25), (CH - 10, 33), (CH - 10, 34), (CH - 10, 700),
                     (CH - 20, 20), (0, CH), (0, LDS + 1), (10, 1500)):
        rec = d.pad(start, start=True) + (d.piece(rng, n) if start else d.word(rng, n))
        arenas.append([d.pad(CH, start=True), rec])
        c = d.cen(arenas[-1])
        ln, path = piece_at(c, CH + start)
        assert ln == n and c[-1]["pieces"] == [] or c[-1]["pieces"][-1][0] == CH + start
        want = ("past" if start + n >= CH + HR - 8 else "long_global" if n > LDS else "long_lds" if n > WAVE else
                "lane" if n <= LANE else "wave")
        assert path == want, (start, n, path)
    return arenas


# ---- rec_local / chunk_cnt after a long piece ------------------------------------------------------------
@case
def fixup_two_long_pieces(d):
    """One chunk holds two long pieces (70 and 90 bytes), each its own record and each followed
    by short records in the same chunk: their local offsets grow by both pieces' extra ids."""
    rng = d.rng("fixup_two")
    blobs = [d.word(rng, 30), d.word(rng, 70)] + [d.word(rng, rng.randint(1, 9)) for _ in range(4)]
    blobs += [d.word(rng, 90)] + [d.word(rng, rng.randint(1, 20)) for _ in range(5)]
    used = sum(map(len, blobs))
    blobs.append(d.pad(CH - used, start=True))
    c = d.cen(blobs)
    assert len(c) == 1 and piece_at(c, 30) == (70, "long_lds")
    assert piece_at(c, 100 + sum(map(len, blobs[2:6]))) == (90, "long_lds")
    assert len(d.t.encode_word(blobs[1])) > 1 and len(d.t.encode_word(blobs[6])) > 1
    return [[*blobs, *blobs]]  # (a second chunk: chunk_cnt and rec_local of chunk 1 as well)


@case
def fixup_long_piece_is_last(d):
    """A long piece that is the last record of its chunk (ending at c1, and running into the next
    chunk), and long pieces in three consecutive chunks."""
    rng = d.rng("fixup_last")
    a = [d.pad(CH - 124, start=True), d.word(rng, 124), d.pad(CH, start=True)]
    b = [d.pad(CH - 100, start=True), d.word(rng, 300), d.pad(CH - 200, start=True)]
    e = []
    for _ in range(3):
        e += [d.word(rng, 10), d.word(rng, 400), d.word(rng, 3), d.word(rng, 500), d.pad(CH - 913, start=True)]
    blobs = a + b + e
    c = d.cen(blobs)
    assert piece_at(c, CH - 124) == (124, "long_lds") and c[0]["pieces"][-1][0] == CH - 124
    assert piece_at(c, 3 * CH - 100) == (300, "past") and all(paths(ch, "long_lds") == 2 for ch in c[4:7])
    return [blobs]


# ---- copy-out ------------------------------------------------------------------------------------------
@case
def copyout_unpacked(d):
    """Chunks above 2 * WIN / 4 list entries (words outside the merge alphabet: one id a byte):
    the scattered stores, from lane and from wave words."""
    rng = d.rng("copyout_unpacked")
    blobs = []
    for n in (LANE, 20):
        body = b"x" + b"".join(d.piece(rng, n, OUT) for _ in range((CH - 1) // n))
        blobs.append(d.finish(body))
    c = d.cen(blobs)
    assert all(ch["entries"] > PACKED + 400 for ch in c)
    return [blobs]


@case
def copyout_at_the_limit(d):
    """2 * WIN / 4 entries exactly (the packed stores' last size) and one more (unpacked): a long
    piece is one entry of the chunk's list whatever it ends as."""
    rng = d.rng("copyout_limit")
    blobs = []
    for target in (PACKED, PACKED + 1):
        n_lane = (target - 4) // LANE
        r = target - 2 - n_lane * LANE  # 2..LANE + 1 entries from one more word; "x" and the long piece: one each
        body = b"x" + b"".join(d.piece(rng, LANE, OUT) for _ in range(n_lane)) + d.piece(rng, r, OUT)
        body += d.piece(rng, CH - len(body), OUT)
        blobs.append(body)
    c = d.cen(blobs)
    assert [ch["entries"] for ch in c] == [PACKED, PACKED + 1] and all(ch["ids"] == CH for ch in c)
    assert all(ch["pieces"][-1][2] == "long_lds" for ch in c)
    return [blobs]


@case
def copyout_below_the_limit(d):
    """A chunk of random words of the merge alphabet: far fewer entries than bytes, packed."""
    rng = d.rng("copyout_below")
    body = b"a" + b"".join(d.piece(rng, rng.randint(2, 40)) for _ in range(45))
    c = d.cen([d.finish(body)])
    assert 100 < c[0]["entries"] < PACKED
    return [[d.finish(body)]]


# ---- the word table's tail compare ---------------------------------------------------------------------
def _as_records(d, words):
    """Each word its own record (a word with a leading space follows one filler letter)."""
    return [(b"a" + w if w[:1] == b" " else w) + d.fill for w in words]


@case
def table_accept(d):
    """Vocabulary strings of 17..40 bytes that encode to themselves, as whole pre-tokens."""
    blobs = _as_records(d, d.long_self)
    c = d.cen(blobs)
    hits = [n for ch in c for _, n, path in ch["pieces"] if path == "hit" and n >= 17]
    assert len(hits) == len(d.long_self) >= mv.MIN_LONG_SELF and max(hits) > 32
    return [blobs]


def _near(d, s):
    """s with one ASCII byte past the 16th changed to another letter of the alphabet."""
    out = []
    for k in range(16, len(s)):
        if s[k] < 0x80:
            for l in b"abc":
                if l != s[k]:
                    out.append(s[:k] + bytes([l]) + s[k + 1:])
    return [w for w in out if w not in d.t.ids]


@case
def table_near_misses(d):
    """The same length and first 16 bytes as such a string, one later byte changed: a miss
    (these name other slots than the string does: see table_reject)."""
    words = [w for s in d.long_self for w in _near(d, s)[:3]]
    blobs = _as_records(d, words)
    c = d.cen(blobs)
    miss = [n for ch in c for _, n, path in ch["pieces"] if path == "wave" and n >= 17]
    assert len(miss) == len(words) >= 2 * mv.MIN_LONG_SELF
    return [blobs]


def collisions(d):
    """[(token, string, j)]: the string has the token's length and all but its last three bytes
    (ASCII letters instead), is no vocabulary string, and one of the two slots its hash names
    equals the token's slot j (1 or 2) on COLLIDE_BITS bits.  The table builder put the token in
    one of its two slots and the probe reads both of the string's, so of a token's j = 1 and
    j = 2 strings one finds the token's header (length, first 16 bytes) and only the compare of
    the bytes past 16 rejects it -- whichever slot the builder chose.  For every long
    self-encoding token whose last three bytes lie in its last 16-byte block behind whole
    letters: the first string of either kind in a fixed enumeration.  The hash is
    tests/golden/make_t5_long_piece_vocab.py's restatement of common.hpp's (the BPE word table
    uses the same piece_hash and cuckoo slots, assets.cpp)."""
    alpha = [c for c in range(0x41, 0x7B) if chr(c).isalpha()]
    mask = (1 << COLLIDE_BITS) - 1
    out = []
    for s in d.long_self:
        n = len(s)
        b0 = 16 * ((n - 1) // 16)
        if n < 19 or n - 3 < max(b0, 16):
            continue
        try:
            s[:n - 3].decode()
        except UnicodeDecodeError:
            continue
        mine = lp.piece_slots(s, COLLIDE_BITS)
        h0 = lp.ph_init(n, 0)
        for k in range(0, b0, 4):
            h0 = lp.ph_mix(h0, int.from_bytes(s[k:k + 4], "little"))
        found = {}
        for t0 in alpha:
            for t1 in alpha:
                for t2 in alpha:
                    blk = (s[b0:n - 3] + bytes([t0, t1, t2])).ljust(16, b"\0")
                    h = h0
                    for i in range(4):
                        h = lp.ph_mix(h, int.from_bytes(blk[4 * i:4 * i + 4], "little"))
                    h = lp.ph_final(h)
                    theirs = (lp.cuckoo_slot1(h, mask), lp.cuckoo_slot2(h, mask))
                    for j in (1, 2):
                        if j not in found and mine[j - 1] in theirs:
                            w = s[:n - 3] + bytes([t0, t1, t2])
                            if w != s and w not in d.t.ids:
                                found[j] = w
                if len(found) == 2:
                    break
            if len(found) == 2:
                break
        out += [(s, w, j) for j, w in sorted(found.items())]
    return out


@case
def table_reject(d):
    """Strings whose hash names a long vocabulary string's slot and whose header matches it: the
    tail compare's reject side.  Every token used has a string for its first and one for its
    second slot, so the slot it occupies is probed whichever the builder chose."""
    col = collisions(d)
    kinds = {}
    for s, w, j in col:
        assert len(w) == len(s) and w[:16] == s[:16] and w != s and not d.t.is_self(w)
        assert lp.piece_slots(s, COLLIDE_BITS)[j - 1] in lp.piece_slots(w, COLLIDE_BITS)
        kinds.setdefault(s, set()).add(j)
    assert len(kinds) >= 2 and all(k == {1, 2} for k in kinds.values())
    blobs = _as_records(d, [w for _, w, _ in col] + list(kinds))
    c = d.cen(blobs)
    assert sum(paths(ch, "wave") for ch in c) == len(col)
    return [blobs]


# ---- sweep ---------------------------------------------------------------------------------------------
SWEEP = (2, 3, 11, 12, 13, 16, 17, 32, 33, 63, 64, 65, 128, 129, 1024, 1025, 2000)


def _sweep(d, k):
    rng = d.rng(f"sweep{k}")
    blobs, seen = [], set()
    for n in SWEEP:
        for _ in range(2):
            off = rng.randint(1, CH - 1)
            blobs.append(d.at(off, d.piece(rng, n), d.fill * 2))
    rng.shuffle(blobs)
    for ch in d.cen(blobs):
        seen |= set(paths(ch))
    assert seen >= set(bpe_census.PATHS) - {"long_global"}  # (known-length global pieces: global_lengths)
    return [blobs]


@case
def sweep_a(d):
    """Every length of SWEEP, two random words an arena, at random byte offsets of their chunk."""
    return _sweep(d, 0)


@case
def sweep_b(d):
    return _sweep(d, 1)


@case
def sweep_c(d):
    return _sweep(d, 2)


# ---- the tests -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=mv.SEEDS)
def dev(request, native_lib, tmp_path_factory):
    path = mv.write(request.param, str(tmp_path_factory.mktemp(f"bpe_merge_{request.param}")))
    return Dev(request.param, path)


def arenas_of(d, name):
    if name not in d.built:
        d.built[name] = CASES[name](d)
    return d.built[name]


@pytest.mark.parametrize("name", list(CASES))
def test_case(torch, dev, name):
    for blobs in arenas_of(dev, name):  # (the census conditions are asserted while building)
        dev.check(torch, blobs)


def test_every_path_is_reached(dev):
    """Pieces per path over all cases of this table; no path, long-kernel form or copy-out form
    may be reached by none."""
    acc, packed, unpacked = {}, 0, 0
    for name in CASES:
        for blobs in arenas_of(dev, name):
            c = dev.cen(blobs)
            bpe_census.count_paths(c, acc)
            packed += sum(1 for ch in c if ch["entries"] <= PACKED)
            unpacked += sum(1 for ch in c if ch["entries"] > PACKED)
            for ch in c:
                for f in ch["form"].values():
                    acc["form/" + f] = acc.get("form/" + f, 0) + 1
    print(f"table {dev.t.seed}: pieces per path {dict(sorted(acc.items()))}; chunks packed {packed}, "
          f"unpacked {unpacked}")
    for k in bpe_census.PATHS + ("past/lds", "past/global", "form/lds", "form/global"):
        assert acc.get(k, 0) > 0, k
    assert packed > 0 and unpacked > 0


def test_error_flag_is_reported_and_reads_zero(torch, dev):
    """d_tokenize_errors is a device pointer for the gpt2 tokenizer and reads 0 after a call with
    long pieces and after one with none (launch_bpe_chunks clears it with the long-piece counter;
    before, it was never handed out and never initialised).  No input can set it, so that a set
    flag is cleared by the next call is not shown here."""
    for blobs in ([dev.finish(dev.word(dev.rng("err"), 3000))], [dev.pad(CH, start=True)]):
        res = run(torch, dev.db, blobs)
        assert res.r.d_tokenize_errors and res.tokenize_errors() == 0
