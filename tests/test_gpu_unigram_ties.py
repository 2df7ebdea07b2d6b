"""GPU parity for the Unigram tokenizer on tied and one-ulp-apart piece scores.

Every device path that settles a word -- the host-built word table, k_unigram_viterbi<false>
(narrow jobs), k_unigram_viterbi<true> (wide jobs), the medium-word arena, k_unigram_long
<20|32|64> in two stages, k_unigram_huge, the fused small push -- has to reproduce `tokenizers`'
Viterbi exactly: candidates by start ascending then length ascending, a node replaced only by a
strictly better candidate, the start's unk last, f64 sums taken as `score + best_till_here`,
the f64 score restored from the stored f32 and the piece's one-ulp mark (uni_score64).  On the
proxy vocabulary two segmentations almost never have equal sums, so none of that decides an
id.  On the vocabularies of tests/golden/make_t5_tied_vocab.py it does: every score -8 (flat),
a grid of 2.0 (g2), the grids of 2.0 and 0.5 with a seeded f64-ulp nudge (u2, u05), on the
proxy and on the long-piece variants v19 / v32 / v64.

The cases come from the builders of tests/uni_tie_cases.py.  tests/test_t5_tied_scores.py runs
the same builders without a device and shows, per case and vocabulary, that a plain model of
the Viterbi equals the oracle on the case's words and that its wrong variants (`>=`, f32-only
scores, reversed sums) change the ids of a stated number of them -- so a kernel wrong in one of
those ways fails here.  Every case
  * asserts its census condition first (tests/uni_census.py: which path takes the words; the
    classification does not depend on scores);
  * compares every record's ids with the C oracle, which that module pins to `tokenizers` on
    these vocabularies;
  * asserts the device reported no tokenize error.
One DeviceBatcher per vocabulary (module scope), CLM rows with min_ids=0 and S=2048, arenas of
at most 64 KiB, records of whole 1 KiB chunks.
"""
import numpy as np
import pytest

import oracle_lib
import uni_tie_cases as tc
from streaming_data_loader_amd import batcher as Bt
from streaming_data_loader_amd import native
from streaming_data_loader_amd.device import DeviceBatcher
from test_gpu_span import oracle_span_rows, run, torch  # noqa: F401  (the module-scoped torch fixture)
from test_gpu_unigram_paths import Dev

pytestmark = pytest.mark.gpu


class TieDev(Dev):
    def __init__(self, path, base, kind):
        super().__init__(path)
        tc.equip(self, path, base, kind)


@pytest.fixture(scope="module")
def devs(native_lib, tmp_path_factory):
    """name -> TieDev: one DeviceBatcher per vocabulary, loaded on first use."""
    class Lazy(dict):
        def __missing__(self, name):
            base, kind = name.split("-")
            self[name] = TieDev(tc.write_vocab(tmp_path_factory.mktemp("t5_" + name), base, kind), base, kind)
            return self[name]
    return Lazy()


@pytest.fixture(scope="module")
def words(devs):
    return tc.Words(devs["proxy-u2"])


@pytest.mark.parametrize("case,name", tc.CASE_PARAMS)
def test_tied_scores(torch, devs, words, case, name):
    """table: word-table hits (the host's Viterbi at load); narrow: k_unigram_viterbi<false>, one
    chunk over UNI_VPC (its losers are long items); wide: k_unigram_viterbi<true>, more than
    PFX_JOBS jobs a chunk; medium: the LDS arena's normalize + narrow DP; long: both stages of
    k_unigram_long<20> (v32 / v64: <32> / <64>); window: a word whose end the window does not
    show; long_variant: 17..48-byte words with the wide Viterbi off; huge: k_unigram_huge;
    unk: characters without a piece, through the medium and long paths."""
    dev = devs[name]
    c = tc.CASES[case][0](dev, words)
    cs, _ = dev.chunks(c.blobs)
    c.census(cs)  # the path the case names
    want = dev.check(torch, c.blobs)
    if dev.new and case in ("wide", "long", "long_variant"):
        assert dev.new & {x for w in want for x in w}  # the oracle's output holds the long pieces


@pytest.mark.parametrize("rng_mode", [0, 1])
def test_span_rows_on_u2(torch, devs, words, rng_mode):
    """Span rows (S=128, B=8) over records of narrow, wide and long words on `u2`, against the
    oracle batcher over the same tokenizer file, in both RNG modes."""
    dev = devs["proxy-u2"]
    S, B_ = 128, 8
    blobs = tc.mixed_records(words, 128)
    db = DeviceBatcher(task=native.SDL_TASK_SPAN, batch_size=B_, sequence_length=S, seed=77, tokenizer=dev.path,
                       avg_span_gap=16.0, avg_span_size=2.0, rng_mode=rng_mode)
    res = run(torch, db, blobs, first_record=5)
    assert res.tokenize_errors() == 0
    G = res.rows()
    ids, am, tt, lab = res.planes(G + (-G) % B_)
    want, errs = oracle_span_rows(dev.tok, blobs, B_, S, 77, first_record=5, rng_mode=rng_mode)
    assert G == want["input_ids"].shape[0] > len(blobs)
    np.testing.assert_array_equal(ids[:G], want["input_ids"])
    np.testing.assert_array_equal(am[:G], want["attention_mask"])
    np.testing.assert_array_equal(lab[:G], want["labels"])
    assert res.label_errors() == errs


def test_single_pushes_on_g2(native_lib, devs, words):
    """The same records one push at a time (clm rows on the t5 tokenizer: the fused small push) on
    `g2`: equal to one bulk call, and both to the oracle batcher's rows."""
    dev = devs["proxy-g2"]
    S, B_, seed = 128, 4, 1234
    texts = tc.mixed_records(words, 64)

    def drain(gt, out):
        while True:
            d = gt.get_working_batch()
            if d is None or not d.rows:
                return out
            out.append(d)

    def make():
        return Bt.GenTokenizer(Bt.ModelType.Gpt2, Bt.BatchConfig(B_, S), Bt.Gpt(), Bt.TokenizerConfig(dev.path),
                               chunk=True, seed=seed)
    a = make()
    per = drain(a, [d for d in (a.create_sync_batch(t) for t in texts) if d is not None])
    b = make()
    one = drain(b, b.create_sync_batches(texts))
    ob = oracle_lib.OracleBatcherEx(oracle_lib.Encoder("t5", dev.tok), oracle_lib.CLM, B_, S, seed=seed)
    want = [r for r in (ob.push(t) for t in texts) if r is not None]
    while True:
        r = ob.flush()
        if r is None:
            break
        want.append(r)
    for key in ("input_ids", "attention_mask", "labels"):
        x = np.concatenate([np.asarray(getattr(d, key))[:d.rows] for d in per])
        y = np.concatenate([np.asarray(getattr(d, key))[:d.rows] for d in one])
        w = np.concatenate([r[key][:r["rows"]] for r in want])
        assert x.shape[0] > len(texts)
        np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(x, w)
