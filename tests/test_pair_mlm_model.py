"""MLM sentence pairs (sdl_config.pair 2..4) without a GPU: csrc/pair_draw.hpp in a stand-alone host
program against the Python model of the draw (pair_mlm_model.py), the draw's own promises and its
statistics, the unmasked NSP / SOP rows against tokenizers' encode(first, second) on the proxy
vocabulary, the model's rows on the edge cases, the config word through the Python layers, and the
refusals sdl_batcher_create makes before it looks for a device."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

import mlm_policy_model as P
import pair_model
import pair_mlm_model as M
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from test_list_index import CSRC, HERE, host_compiler

SEEDS = (20240229, 0xDEADBEEF12345678)
MODES = (M.PAIR_MLM, M.PAIR_MLM_NSP, M.PAIR_MLM_SOP)
ERR_ARG, ERR_UNSUPPORTED = -1, -4


# ---- the header against the model ---------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_draw") / "pair_draw_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "pair_draw_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def ask(exe, lines):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    out = r.stdout.split("\n")
    assert out[-2] == "pair_draw ok" and len(out) == len(lines) + 2
    return [tuple(int(v) for v in l.split()) for l in out[:-2]]


def draw_queries():
    q = []
    for seed in SEEDS:
        for mode in MODES:
            for first in (0, 7, 2**32 - 1, 2**32, 2**32 + 1, 2**32 - 3):
                for n in range(1, 10):  # every r and n_pairs in 1..9
                    q += [(seed, first + r, r, n, mode) for r in range(n)]
            # n_pairs 4096, from a record whose rows cross the high counter word
            q += [(seed, 2**32 - 2048 + r, r, 4096, mode) for r in range(4096)]
    return q


def test_header_draw_equals_the_model(check_exe):
    q = draw_queries()
    got = ask(check_exe, ["D %d %d %d %d %d" % t for t in q])
    want = [M.draw(*t) for t in q]
    assert got == want
    # the three records around the high counter word draw from different blocks
    w = ask(check_exe, ["W %d %d" % (SEEDS[0], rec) for rec in (2**32 - 1, 2**32, 2**32 + 1, 1)])
    assert w == [M.draw_words(SEEDS[0], rec) for rec in (2**32 - 1, 2**32, 2**32 + 1, 1)]
    assert len(set(w)) == 4 and w[1] != M.draw_words(SEEDS[0], 0)
    assert M.draw_words(SEEDS[0], 5) != M.draw_words(SEEDS[1], 5)


def test_header_kept_lengths_equal_the_model(check_exe):
    q = [(na, nb, S - 3) for S in (3, 4, 8, 9, 16, 17, 128) for na in range(0, 2 * S + 2, 1 if S < 20 else 7)
         for nb in range(0, 2 * S + 2, 1 if S < 20 else 5)]
    q += [(2**32 - 1, 2**32 - 1, 2045), (2**32 - 1, 3, 125), (0, 2**32 - 1, 0)]
    got = ask(check_exe, ["K %d %d %d" % t for t in q])
    assert got == [pair_model.kept_lengths(na, nb, M_ + 3) for na, nb, M_ in q]


# ---- the draw's promises and statistics ---------------------------------------------------------
def test_nsp_never_draws_the_rows_own_b():
    for seed in SEEDS:
        for n in (2, 3, 9, 64):
            for first in (0, 1000):
                for r in range(n):
                    f, s, lab = M.draw(seed, first + r, r, n, M.PAIR_MLM_NSP)
                    assert f == 2 * r and s % 2 == 1 and 0 <= s < 2 * n
                    assert (lab == 1) == (s != 2 * r + 1)
    # a call of one pair is never random; of two, a random row takes the other one's B
    assert all(M.draw(SEEDS[0], rec, 0, 1, M.PAIR_MLM_NSP) == (0, 1, 0) for rec in range(400))
    seen = set()
    for rec in range(200):
        for r in (0, 1):
            f, s, lab = M.draw(SEEDS[0], rec, r, 2, M.PAIR_MLM_NSP)
            assert s == (2 * (1 - r) + 1 if lab else 2 * r + 1)
            seen.add((r, lab))
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_sop_swaps_and_pair_2_does_not():
    labs = []
    for r in range(300):
        f, s, lab = M.draw(SEEDS[1], 50 + r, r, 300, M.PAIR_MLM_SOP)
        assert (f, s) == ((2 * r + 1, 2 * r) if lab else (2 * r, 2 * r + 1))
        labs.append(lab)
        assert M.draw(SEEDS[1], 50 + r, r, 300, M.PAIR_MLM) == (2 * r, 2 * r + 1, 0)
    assert 0 < sum(labs) < 300


def test_the_coin_is_fair_and_every_other_example_is_a_source():
    """4096 examples at a fixed seed: the share of label 1 within five standard deviations of a fair
    coin at that count (0.5 +- 0.04 is wider: 5 * 0.5 / sqrt(4096) = 0.039); and over the calls of
    a stream cut into calls of 9, every row position takes every other one's B at least once."""
    n = 4096
    for mode in (M.PAIR_MLM_NSP, M.PAIR_MLM_SOP):
        share = sum(M.draw(SEEDS[0], r, r, n, mode)[2] for r in range(n)) / n
        assert abs(share - 0.5) <= 0.04, share
    # the same coin decides NSP and SOP (one block, word x)
    assert all(M.draw(SEEDS[0], r, r, n, M.PAIR_MLM_NSP)[2] == M.draw(SEEDS[0], r, r, n, M.PAIR_MLM_SOP)[2]
               for r in range(0, n, 17))
    sources = {r: set() for r in range(9)}
    for call in range(n // 9):
        for r in range(9):
            _, s, lab = M.draw(SEEDS[0], 9 * call + r, r, 9, M.PAIR_MLM_NSP)
            if lab:
                sources[r].add((s - 1) // 2)
    for r in range(9):
        assert sources[r] == set(range(9)) - {r}, r
    # ... and within one call of 4096, the sources spread over the whole call
    src = {(M.draw(SEEDS[0], r, r, n, M.PAIR_MLM_NSP)[1] - 1) // 2 for r in range(n)}
    assert min(src) < 64 and max(src) >= n - 64 and len(src) > n // 2


def test_the_draw_depends_on_the_cut_into_calls():
    """The same record in a call of another size, or at another row of its call, may take another
    B; its label (the coin) stays."""
    a = [M.draw(SEEDS[0], rec, rec % 8, 8, M.PAIR_MLM_NSP) for rec in range(400)]
    b = [M.draw(SEEDS[0], rec, rec % 50, 50, M.PAIR_MLM_NSP) for rec in range(400)]
    assert [x[2] for x in a] == [x[2] for x in b]
    assert any(x[2] and (x[1] - 1) // 2 != (y[1] - 1) // 2 for x, y in zip(a[:8], b[:8]))  # (the same rows r = rec)


# ---- the unmasked rows against the library the pair contract is pinned to ------------------------
def random_text(rng):
    alphabet = "abcdefghij klmnop,.;!? ÄéßİＡ中文​\t\n"
    return "".join(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 5, 12, 40, 90, 200])))


@pytest.mark.parametrize("mode", [M.PAIR_MLM_NSP, M.PAIR_MLM_SOP])
@pytest.mark.parametrize("S", [8, 17, 32])
def test_unmasked_rows_match_tokenizers(S, mode):
    import tokenizers
    plain = tokenizers.Tokenizer.from_file(native.BERT_PROXY_TOKENIZER)
    cls, sep = plain.token_to_id("[CLS]"), plain.token_to_id("[SEP]")
    tk = tokenizers.Tokenizer.from_file(native.BERT_PROXY_TOKENIZER)
    tk.enable_truncation(max_length=S, strategy="longest_first")
    tk.enable_padding(length=S)
    rng = random.Random(77 + S)
    pairs = [(random_text(rng), random_text(rng)) for _ in range(120)]
    ids = [(plain.encode(a, add_special_tokens=False).ids, plain.encode(b, add_special_tokens=False).ids)
           for a, b in pairs]
    seed, first = SEEDS[0], 2**32 - 40
    rows, plab, fill = M.unmasked(ids, S, mode, seed, first, cls, sep)
    texts = M.chosen(pairs, mode, seed, first)
    assert 20 < int(plab.sum()) < 100
    for r, (first_text, second_text, lab) in enumerate(texts):
        e = tk.encode(first_text, second_text)
        assert rows[0, r].tolist() == e.ids and rows[2, r].tolist() == e.type_ids
        assert rows[1, r].tolist() == e.attention_mask and sum(e.attention_mask) == fill[r]
        assert lab == plab[r]
        f, s, _ = M.draw(seed, first + r, r, len(pairs), mode)
        if mode == M.PAIR_MLM_SOP:
            assert (first_text, second_text) == (pairs[r][::-1] if lab else pairs[r])
        else:
            assert f == 2 * r and first_text == pairs[r][0] and second_text == pairs[(s - 1) // 2][1]
            assert ((s - 1) // 2 != r) == bool(lab)


# ---- the model's rows ----------------------------------------------------------------------------
def word_ids(n, base=2000):
    return [base + i for i in range(n)]  # whole-word pieces of the proxy vocabulary (asserted below)


def test_model_rows_edge_cases():
    vocab_size, cont, cls, sep = P.proxy_vocab()
    S = 16
    pairs = [([], []), (word_ids(4), []), ([], word_ids(5, 2050)), (word_ids(3), word_ids(40, 2050)),
             (word_ids(30), word_ids(2, 2050)), (word_ids(6), word_ids(7, 2050))]
    for mode in MODES:
        for policy in (1, 2):
            out = M.rows(pairs, S, mode, policy, SEEDS[0], first_record=11, mask_length=S, B=4)
            pl, plab = out["planes"], out["pair_labels"]
            assert pl.shape == (4, 8, S) and plab.shape == (8,)
            # rows nobody filled
            assert (pl[0, 6:] == 0).all() and (pl[1, 6:] == 1).all() and (pl[2, 6:] == 0).all()
            assert (pl[3, 6:] == -100).all() and (plab[6:] == -100).all() and set(plab[:6].tolist()) <= {0, 1}
            plain, _, fill = M.unmasked(pairs, S, mode, SEEDS[0], 11, cls, sep)
            for r in range(6):
                picked = np.nonzero(pl[3, r] != -100)[0]
                l = fill[r]
                cand = [j for j in range(l) if plain[0, r, j] not in (cls, sep)]
                want = P.budget(l, len(cand), S, 150)
                assert set(picked.tolist()) <= set(cand) and len(picked) <= min(want, len(cand))
                if policy == 1:  # (policy 2 may skip a word that no longer fits)
                    assert len(picked) == min(want, len(cand))
                assert (pl[3, r, picked] == plain[0, r, picked]).all()
                assert (pl[1, r] == plain[1, r]).all() and (pl[2, r] == plain[2, r]).all()
                off = np.ones(S, bool)
                off[picked] = False
                assert (pl[0, r, off] == plain[0, r, off]).all()
            if mode == M.PAIR_MLM:  # both empty: [CLS] [SEP] [SEP], no candidate, no pick
                assert pl[0, 0].tolist() == [cls, sep, sep] + [0] * (S - 3) and (pl[3, 0] == -100).all()
                assert pl[2, 0].tolist() == [0, 0, 1] + [0] * (S - 3) and (plab[:6] == 0).all()


def test_masks_are_keyed_by_the_rows_own_index():
    """A row whose second segment is foreign is masked as chunk 0 of its own record, not the
    source's: the picks of a row equal those of the same ids pushed as given at the same index."""
    rng = random.Random(3)
    pairs = [(word_ids(rng.randint(2, 9)), word_ids(rng.randint(2, 9), 2050 + 10 * i)) for i in range(12)]
    S, seed = 32, SEEDS[1]
    nsp = M.rows(pairs, S, M.PAIR_MLM_NSP, 1, seed, first_record=100)
    ch = M.chosen(pairs, M.PAIR_MLM_NSP, seed, 100)
    assert any(lab for _, _, lab in ch)
    given = M.rows([(a, b) for a, b, _ in ch], S, M.PAIR_MLM, 1, seed, first_record=100)
    np.testing.assert_array_equal(nsp["planes"], given["planes"])
    other = M.rows([(a, b) for a, b, _ in ch], S, M.PAIR_MLM, 1, seed, first_record=101)
    assert (other["planes"][3] != given["planes"][3]).any()


# ---- the config word through the layers ----------------------------------------------------------
def test_constants_and_python_layers():
    assert (native.SDL_PAIR_NONE, native.SDL_PAIR_ROWS, native.SDL_PAIR_MLM, native.SDL_PAIR_MLM_NSP,
            native.SDL_PAIR_MLM_SOP) == (0, 1, 2, 3, 4)
    assert B.Mask(19).pair == 0
    for mode in MODES:
        c, kind = B._native_config(B.BatchConfig(4, 16), B.Mask(4, 103, 1, 150, pair=mode), True, 0, 0, 0, 0)
        assert c.pair == mode and kind == "bert" and list(c.reserved)[3] == mode
    c, _ = B._native_config(B.BatchConfig(4, 16), B.Mask(4), True, 0, 0, 0, 0)
    assert c.pair == 0
    ds = B.DataSet("bert", 2, np.zeros((3, 4), np.int32), np.ones((3, 4), np.int32), np.full((3, 4), -100, np.int32),
                   np.zeros((3, 4), np.int32), pair_labels=np.array([1, 0, -100], np.int32),
                   pair_key="sentence_order_label")
    d = ds.to_dict()
    assert list(d) == ["input_ids", "attention_mask", "token_type_ids", "labels", "sentence_order_label"]
    assert d["sentence_order_label"].tolist() == [1, 0]
    plain = B.DataSet("bert", 2, np.zeros((3, 4), np.int32), np.ones((3, 4), np.int32),
                      np.full((3, 4), -100, np.int32), np.zeros((3, 4), np.int32))
    assert list(plain.to_dict()) == ["input_ids", "attention_mask", "token_type_ids", "labels"]
    assert hasattr(B.GenTokenizer, "create_sync_batches_pairs")


def test_header_names_the_modes(tmp_path):
    import shutil
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler found"
    src = tmp_path / "pair_modes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdl_batcher.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %zu %zu %d\\n", SDL_PAIR_NONE, SDL_PAIR_ROWS, SDL_PAIR_MLM,\n'
                   '  SDL_PAIR_MLM_NSP, SDL_PAIR_MLM_SOP, sizeof(sdl_config), offsetof(sdl_config, pair), SDL_ABI_VERSION);\n'
                   '  return 0; }\n')
    exe = tmp_path / "pair_modes"
    subprocess.run([cc, "-std=c11", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split() == \
        ["0", "1", "2", "3", "4", "96", "92", "9"]


# ---- refusals made before a device is looked for -------------------------------------------------
def create_rc(native_lib, task, pair, S=16, mask_policy=1, rng_mode=0):
    c = native.default_config(task)
    c.batch_size, c.sequence_length, c.pair = 4, S, pair
    c.mask_length = min(c.mask_length, 2)
    c.mask_policy, c.rng_mode = mask_policy, rng_mode
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), native.BERT_PROXY_TOKENIZER.encode(), native.DATA_DIR.encode(),
                                       ctypes.byref(h))
    msg = native_lib.sdl_last_error().decode() if rc else ""
    if h.value:
        native_lib.sdl_batcher_destroy(h)
    return rc, msg


def test_config_refusals(native_lib):
    for mode in MODES:
        for task in (native.SDL_TASK_CLM, native.SDL_TASK_SPAN, native.SDL_TASK_MULTI_LABEL,
                     native.SDL_TASK_SINGLE_CLASS):
            rc, msg = create_rc(native_lib, task, mode, mask_policy=0)
            assert rc == ERR_ARG and "pair" in msg, (mode, task, msg)
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, mask_policy=0)
        assert rc == ERR_UNSUPPORTED and "pair" in msg and "mask_policy 0" in msg
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, rng_mode=1)
        assert rc == ERR_UNSUPPORTED and "pair" in msg and "rng_mode" in msg
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, S=2)
        assert rc == ERR_ARG and "pair" in msg and "sequence_length >= 3" in msg
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, mode, S=2049)
        assert rc == ERR_ARG and "pair" in msg and "2048" in msg
        c = native.default_config(native.SDL_TASK_MLM)
        c.batch_size, c.sequence_length, c.pair, c.mask_policy = 4, 16, mode, 1
        m = ctypes.c_void_p()
        devs = (ctypes.c_int32 * 1)(0)
        assert native_lib.sdl_multi_create(ctypes.byref(c), native.BERT_PROXY_TOKENIZER.encode(),
                                           native.DATA_DIR.encode(), devs, 1, ctypes.byref(m)) == ERR_UNSUPPORTED
        assert "pair" in native_lib.sdl_last_error().decode() and not m.value
    for bad in (5, 7, -1):
        assert create_rc(native_lib, native.SDL_TASK_MLM, bad)[0] == ERR_ARG
    # a valid pair-mlm config passes every check made before the device is looked for
    import torch
    if not torch.cuda.is_available():
        rc, msg = create_rc(native_lib, native.SDL_TASK_MLM, native.SDL_PAIR_MLM_NSP)
        assert rc == -5 and "no HIP device" in msg
