"""Tied and one-ulp-apart Unigram scores on the CPU: the vocabularies, the oracle against
`tokenizers` on them, and what the device cases of tests/test_gpu_unigram_ties.py can notice.

tests/golden/make_t5_tied_vocab.py rewrites the scores of the t5 proxy (and of its long-piece
variants) so that segmentations tie: every score -8 (`flat`), a grid of 2.0 or 0.5 (`g2`,
`g05`), the grids with a seeded -1 / 0 / +1 f64-ulp nudge (`u2`, `u05`).  On such vocabularies
the ids depend on what `tokenizers`' Viterbi does with equal sums -- visit order, strict `>`,
the unk last, the association of the f64 additions, the one-ulp mark of a score -- which the
proxy's 32,100 distinct scores never ask for.

Here, without a GPU:
  * the generator's contract (only ids 3..31999 change, the grid, the nudges the loader takes);
  * the C oracle equals `tokenizers` on the seven vocabularies the device tests use;
  * the host loader accepts them;
  * every device case, from the builders of tests/uni_tie_cases.py the GPU tests call too: its
    census condition, the plain model (tests/unigram_plain_model.py) equal to the oracle on every
    guard word, and the number of guard words on which the model's wrong variants -- `>=`
    relaxation, f32-only scores, sums from the last piece -- change the ids.  A case whose wrong
    variants change nothing would pass on a wrong kernel; the thresholds below say what each
    case has to be able to notice, and the counts are printed (run with -s).
"""
import json
import math
import random
import struct

import pytest

import make_t5_long_piece_vocab as lp
import make_t5_tied_vocab as tv
import oracle_lib
import uni_tie_cases as tc
from test_t5_long_pieces import piece_texts

NAMES = [f"{b}-{k}" for b, k in tc.VOCABS]


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    """name -> Host, built on first use."""
    class Lazy(dict):
        def __missing__(self, name):
            base, kind = name.split("-")
            self[name] = tc.Host(tc.write_vocab(tmp_path_factory.mktemp("t5_" + name), base, kind), base, kind)
            return self[name]
    return Lazy()


@pytest.fixture(scope="module")
def words(hosts):
    return tc.Words(hosts["proxy-u2"])


# ---- the generator ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", tv.KINDS)
def test_only_the_ordinary_scores_change(kind):
    with open(lp.TEMPLATE, encoding="utf-8") as f:
        ref = json.load(f)
    tok = tv.build(kind)
    rv, v = ref["model"]["vocab"], tok["model"]["vocab"]
    assert [p for p, _ in v] == [p for p, _ in rv]
    assert v[:3] == rv[:3] and v[32000:] == rv[32000:] and len(v) == 32100
    ref["model"]["vocab"] = tok["model"]["vocab"] = None
    assert tok == ref  # normalizer, pre-tokenizer, template, added tokens: untouched
    sc = [s for _, s in v[3:32000]]
    assert all(s < 0 for s in sc)
    if kind == "flat":
        assert set(sc) == {-8.0}
        return
    step = tv.STEP[kind]
    on_grid = [tv.grid(s, step) for _, s in rv[3:32000]]
    assert all(g % step == 0 and g <= -step for g in on_grid)
    d = [_bits(s) - _bits(g) for s, g in zip(sc, on_grid)]
    if kind in ("g2", "g05"):
        assert set(d) == {0}
        assert len(set(sc)) <= 40  # few distinct values: ties are the rule
    else:
        assert set(d) == {-1, 0, 1} and min(d.count(x) for x in (-1, 0, 1)) > 9000
        # what the loader reads back (serde_json's parse of the text json.dump writes) is
        # negative and within one f64 ulp of an f32, and the nudges survive the parse
        read = [oracle_lib.json_number(repr(s)) for s in sc]
        assert all(y < 0 and abs(_bits(y) - _bits(_f32(y))) <= 1 for y in read)
        assert sum(y != _f32(y) for y in read) > 18000
    assert tv.dropped(kind) < 0.01 * len(sc)
    print(f"{kind}: {tv.dropped(kind)} nudges dropped, {len(set(sc))} distinct scores")


def test_unk_score_is_on_the_grid():
    """min - 10 is a grid value on g2 (a path through an unk can tie with one through pieces);
    on u2 it is that value or an f64 neighbour."""
    g2 = min(s for _, s in tv.build("g2")["model"]["vocab"]) - 10.0
    u2 = min(s for _, s in tv.build("u2")["model"]["vocab"]) - 10.0
    assert g2 % 2.0 == 0 and abs(_bits(u2) - _bits(g2)) <= 1
    assert tv.build("flat")["model"]["vocab"][5][1] - 10.0 == -18.0


@pytest.mark.parametrize("base", ["v19", "v32", "v64"])
def test_long_piece_bases_keep_their_pieces(base):
    a, b = lp.build(base)["model"]["vocab"], tv.build("g2", base)["model"]["vocab"]
    assert [p for p, _ in a] == [p for p, _ in b] and a[:3] == b[:3] and a[32000:] == b[32000:]
    assert all(s % 2.0 == 0 and s < 0 for _, s in b[3:32000]) and tv.dropped("u2", base) < 320


# ---- the oracle against tokenizers ----------------------------------------------------------------

def tie_texts(ctx, seed=300, n=300):
    """Seeded texts of concatenated-piece words of 3..600 bytes; runs of one character; words with
    characters that have no piece."""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        k = rng.randint(1, 12)
        lens = [rng.choice((rng.randint(3, 16), rng.randint(17, 48), rng.randint(49, 128), rng.randint(3, 600)))
                for _ in range(k)]
        out.append(" ".join(ctx.cat(rng, m) for m in lens))
    out += ["=" * 52, " ".join("=" * m for m in range(1, 70)), " ".join("a" * m for m in (1, 2, 3, 5, 16, 17, 48, 49, 130, 600)),
            " ".join(c * m for c in "e-0_x" for m in (4, 9, 23, 77))]
    out += [" ".join(tc.accented(ctx, rng, tc.NO_PIECE + tc.WITH_PIECE, 4, 60, 40)) for _ in range(10)]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oracle_matches_tokenizers_on_tied_scores(hosts, records, name):
    tokenizers = pytest.importorskip("tokenizers")
    ctx = hosts[name]
    ref = tokenizers.Tokenizer.from_file(ctx.path)
    texts = list(records) + tie_texts(ctx)
    if ctx.base != "proxy":
        texts += piece_texts(ctx.base)
    assert len(records) == 50
    used = n_ids = 0
    bad = []
    for t in texts:
        want = ref.encode(t).ids
        got = ctx.tok.encode(t)
        n_ids += len(want)
        used += sum(1 for i in want if i in ctx.new)
        if got != want:
            bad.append((t[:60], want[:8], got[:8]))
    print(f"{name}: {len(bad)} of {len(texts)} texts differ, {n_ids} ids, {used} uses of the new long pieces")
    assert not bad, f"{len(bad)} of {len(texts)} texts differ, e.g. {bad[:2]}"
    assert ctx.base == "proxy" or used > 0, "no text used a new long piece"


@pytest.mark.parametrize("name", NAMES)
def test_host_loader_accepts_the_tied_vocabularies(native_lib, hosts, name):
    from streaming_data_loader_amd import native
    info = native.tokenizer_info(hosts[name].path)
    assert info.kind == 2 and info.eos_id == 1 and info.unk_id == 2 and info.vocab_size == 32100


# ---- what the device cases can notice ----------------------------------------------------------------

def test_searched_words(words):
    """Words on which the f32-only and the reversed-sum variants of the model change the ids are
    1..2 % of seeded words on `u2`; the searches have to find the few each list is given."""
    for name, _, _, _, n_f32, n_rev in tc.Words.CLASSES:
        f = words.found[name]
        print(f"{name}: f32-only {len(f['f32'][0])} found in {f['f32'][1]} draws, "
              f"reversed sum {len(f['reverse_sum'][0])} in {f['reverse_sum'][1]}")
        assert len(f["f32"][0]) == n_f32 and len(f["reverse_sum"][0]) == n_rev
    assert len(words.narrow_over) > tc.K["UNI_VPC"]


# The `>=` variant has to change at least 5 % of a case's guard words and at least 5 of them on
# flat, g2 and u2 (measured: 9..90 %); on u05 (a finer grid: fewer ties) at least one.
# On u2 the f32-only variant has to change >= 3 narrow, >= 3 wide, >= 1 word-table, long and huge
# words, the reversed sum >= 1 narrow and wide word.
F32_MIN = {"narrow": 3, "wide": 3, "table": 1, "long": 1, "huge": 1}
REV_MIN = {"narrow": 1, "wide": 1}


@pytest.mark.parametrize("case,name", tc.CASE_PARAMS)
def test_case_census_and_guards(hosts, words, case, name):
    ctx = hosts[name]
    c = tc.CASES[case][0](ctx, words)
    assert sum(map(len, c.blobs)) <= tc.ARENA_MAX
    cs, _ = ctx.chunks(c.blobs)
    c.census(cs)
    for w in c.guard:
        assert ctx.tok.normalize(w) == w  # the plain model does not normalize
    n = tc.guard_counts(ctx, c.guard)
    print(f"{name} {case} [{c.path}]: {len(c.guard)} guard words; `>=` changes {n['strict']}, "
          f"f32-only {n['f32']}, reversed sum {n['reverse_sum']}")
    if case == "table" and ctx.kind == "flat":
        # with every score -8 the fewest pieces win: "▁w" alone beats any split, and no w was found
        # whose "w," or "w." has two splits into two pieces -- on flat this case only checks the ids
        assert n["strict"] == 0
    elif ctx.kind == "u05":
        assert n["strict"] >= 1
    else:
        assert n["strict"] >= max(5, math.ceil(0.05 * len(c.guard)))
    if ctx.kind == "u2" and ctx.base == "proxy":
        assert n["f32"] >= F32_MIN.get(case, 0) and n["reverse_sum"] >= REV_MIN.get(case, 0)
    if ctx.kind in ("flat", "g2"):
        assert n["f32"] == n["reverse_sum"] == 0  # grid sums are exact in f32 and in any order
    if ctx.new and case in ("wide", "long_variant", "long"):
        assert ctx.new & {i for w in c.guard for i in ctx.model.encode_word(w)}  # the long pieces win
