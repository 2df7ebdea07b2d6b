"""T5's span corruption (sdl_config.span_policy 1) without a GPU: the Python model of the contract
(span_noise_model.py) against known answers that depend on no random draw and its own invariants,
the two config words through the C header, the ctypes mirror and the Python layers, the refusals
sdl_batcher_create makes before it looks for a device, and csrc/span_noise.hpp in a stand-alone
host program under the host sanitizers (forced equal keys included)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import span_noise_model as M
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native
from test_list_index import CSRC, HERE, host_compiler

SEED = 1234


# ---- the model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S, n_rows, n_spans, n_noise", [(64, 377, 1073, 3534), (128, 199, 1074, 3366),
                                                         (512, 63, 1143, 3404)])
def test_known_answers_on_the_fixture(S, n_rows, n_spans, n_noise):
    """The fixture's records through the t5 proxy at 150 per mille, mean 3.0: rows, spans and noise
    ids (none depends on a draw).  rows() asserts the round trip and a_s, b_s >= 1 on every row."""
    planes, info = M.rows(M.fixture_records(), S, 150, 3.0, SEED)
    assert (len(info), sum(len(i["a"]) for i in info), sum(sum(i["b"]) for i in info)) == (n_rows, n_spans, n_noise)
    assert min(i["n"] for i in info) == 4  # (the edge rows of the GPU test have to be synthetic)
    ids, am, lab = planes["input_ids"], planes["attention_mask"], planes["labels"]
    for g, i in enumerate(info):
        t, m = M.counts(i["n"], 150, 3.0)
        L = i["n"] - t + m
        assert am[g].tolist() == [1] * L + [0] * (S - L) and (ids[g, L:] == 0).all() and (ids[g, :L] != 0).all()
        assert int((lab[g] != -100).sum()) == t + m + 1 and (lab[g, t + m + 1:] == -100).all()
        assert lab[g, t + m] == M.extra_ids()[m]


def test_counts_table_of_the_contract():
    """The capacity table of the contract: (labels needed, sentinels needed) by a full row."""
    assert M.counts(512, 150, 3.0) == (77, 26) and M.capacity(512, 150, 3.0) == (104, 27)
    assert M.counts(64, 150, 3.0) == (10, 3) and M.capacity(64, 150, 3.0) == (14, 4)
    assert M.counts(2048, 150, 3.0) == (307, 102) and M.capacity(2048, 150, 3.0) == (410, 103)
    assert M.counts(2048, 100, 3.0) == (205, 68) and M.capacity(2048, 100, 3.0) == (274, 69)
    assert [M.counts(n, 150, 3.0) for n in range(5)] == [(0, 0), (0, 0), (1, 1), (1, 1), (1, 1)]
    assert M.counts(3, 500, 1.0) == (2, 1)  # m <= n - t


def test_rows_of_one_two_and_three_ids():
    eos, x = M.tok().eos, M.extra_ids()
    i, am, lab, (a, b) = M.row([eos], 64, SEED, 0, 5, 150, 3.0)
    assert (a, b) == ([], []) and i[:2].tolist() == [eos, 0] and am[:2].tolist() == [1, 0]
    assert lab[:2].tolist() == [x[0], -100]
    i, am, lab, (a, b) = M.row([7, 8], 64, SEED, 0, 0, 150, 3.0)
    assert (a, b) == ([1], [1]) and i[:3].tolist() == [7, x[0], 0] and lab[:4].tolist() == [x[0], 8, x[1], -100]
    i, am, lab, (a, b) = M.row([7, 8, 9], 64, SEED, 0, 0, 500, 1.0)
    assert (a, b) == ([1], [2]) and i[:3].tolist() == [7, x[0], 0] and lab[:5].tolist() == [x[0], 8, 9, x[1], -100]


def test_compositions_are_uniform_enough():
    """Every one of the C(5, 2) = 10 compositions of 6 into 3 parts turns up over 400 rows."""
    seen = {tuple(M.composition(SEED, rec, 0, M.NOISE_DOMAIN, 6, 3)) for rec in range(400)}
    assert len(seen) == 10 and all(sum(c) == 6 and min(c) >= 1 for c in seen)
    assert M.composition(SEED, 3, 0, M.NOISE_DOMAIN, 6, 3) != M.composition(SEED, 3, 0, M.KEEP_DOMAIN, 6, 3) or \
        M.composition(SEED, 4, 0, M.NOISE_DOMAIN, 6, 3) != M.composition(SEED, 4, 0, M.KEEP_DOMAIN, 6, 3)


@pytest.mark.parametrize("target", [3, 4, 9, 63, 64, 65, 71])
def test_grown_records_hit_their_id_count(target):
    assert len(M.record_ids(M.grown_record(target))) == target


# ---- the config words -------------------------------------------------------------------------------
def test_header_layout_from_a_c_compiler(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler found"
    src = tmp_path / "span_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdl_batcher.h"\n'
                   'int main(void) { sdl_config c;\n'
                   'printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(sdl_config), offsetof(sdl_config, span_policy), '
                   'offsetof(sdl_config, span_noise_per_mille), offsetof(sdl_config, reserved), sizeof(c.reserved), '
                   'SDL_SPAN_REFERENCE, SDL_SPAN_T5); return 0; }\n')
    exe = tmp_path / "span_layout"
    subprocess.run([cc, "-std=c11", "-Wall", "-Werror", "-I", os.path.join(os.path.dirname(HERE), "include"), str(src),
                    "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [96, 84, 88, 84, 12, 0, 1]


def test_ctypes_mirror_and_defaults(native_lib):
    assert ctypes.sizeof(native.Config) == 96
    assert native.Config.span_policy.offset == 84 and native.Config.span_noise_per_mille.offset == 88
    assert native.Config.reserved.offset == 80 and native.Config.reserved.size == 16
    assert (native.SDL_SPAN_REFERENCE, native.SDL_SPAN_T5) == (0, 1)
    for task in range(5):
        c = native.default_config(task)
        assert (c.span_policy, c.span_noise_per_mille) == (0, 0) and list(c.reserved) == [0, 0, 0, 0]
    c = native.Config()
    c.span_policy, c.span_noise_per_mille = 1, 150
    assert list(c.reserved) == [0, 1, 150, 0]


def test_rust_mirror_of_the_config_matches_the_ctypes_one():
    """INTEGRATION.md's `SdlConfig` field by field against native.Config: names, types, offsets.
    (test_integration_ffi.py reads the header's `typedef struct name { ... } name;` definitions with
    a pattern that takes flat field lists only; sdl_config, with its union, is declared as a struct
    and a typedef apart and is checked here instead.)"""
    from test_integration_ffi import header_api, rust_api
    assert "SdlConfig" not in header_api()[0]
    sizes = {"i32": (4, ctypes.c_int32), "u64": (8, ctypes.c_uint64), "f64": (8, ctypes.c_double)}
    at = 0
    for name, rtype in rust_api()[0]["SdlConfig"]:
        if rtype.startswith("["):
            base, n = rtype[1:-1].split(";")
            size, ct = sizes[base.strip()][0] * int(n), None
        else:
            size, ct = sizes[rtype]
        at = -(-at // min(size, 8)) * min(size, 8) if ct else at
        if name == "reserved":  # the word behind the two span words
            assert (at, size) == (92, 4)
        else:
            f = getattr(native.Config, name)
            assert (f.offset, f.size) == (at, size), name
            assert dict(native.Config._fields_ + native._PackWord._fields_)[name] is ct, name
        at += size
    assert at == ctypes.sizeof(native.Config) == 96


def test_python_layers_set_the_words(native_lib):
    c, kind = B._native_config(B.BatchConfig(4, 512), B.Span(16.0, 3.0, policy=1, noise_per_mille=150), True, 0, 0, 0, 0)
    assert (c.span_policy, c.span_noise_per_mille, c.avg_span_size, c.task, kind) == (1, 150, 3.0, native.SDL_TASK_SPAN, "t5")
    c, _ = B._native_config(B.BatchConfig(4, 512), B.Span(16.0, 2.0), True, 0, 0, 0, 0)
    assert (c.span_policy, c.span_noise_per_mille) == (0, 0)
    c, _ = B._native_config(B.BatchConfig(4, 512), B.Span(16.0, 3.0), True, 0, 0, 0, 0, span_policy=1,
                            span_noise_per_mille=100)
    assert (c.span_policy, c.span_noise_per_mille) == (1, 100)
    assert (B.Span().policy, B.Span().noise_per_mille) == (0, 0)


# ---- the refusals, before a device is looked for ------------------------------------------------------
def create_rc(native_lib, **fields):
    task = fields.pop("task", native.SDL_TASK_SPAN)
    c = native.default_config(task)
    for k, v in fields.items():
        setattr(c, k, v)
    tokenizer = {native.SDL_TASK_MLM: native.BERT_PROXY_TOKENIZER, native.SDL_TASK_CLM: native.GPT2_PROXY_TOKENIZER}.get(
        task, native.T5_PROXY_TOKENIZER if task == native.SDL_TASK_SPAN else native.BERT_PROXY_TOKENIZER)
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), tokenizer.encode(), native.DATA_DIR.encode(), ctypes.byref(h))
    if h:
        native_lib.sdl_batcher_destroy(h)
    return rc, native_lib.sdl_last_error().decode()


T5 = dict(span_policy=1, span_noise_per_mille=150, avg_span_size=3.0, sequence_length=512)
ARG, UNSUPPORTED = -1, -4


@pytest.mark.parametrize("fields, code, words", [
    (dict(T5, span_policy=2), ARG, ["span_policy"]),
    (dict(T5, span_policy=-1), ARG, ["span_policy"]),
    (dict(span_policy=7), ARG, ["span_policy"]),
    (dict(T5, task=native.SDL_TASK_MLM), ARG, ["span_policy"]),
    (dict(T5, task=native.SDL_TASK_CLM), ARG, ["span_policy"]),
    (dict(T5, task=native.SDL_TASK_MULTI_LABEL), ARG, ["span_policy"]),
    (dict(T5, span_noise_per_mille=0), ARG, ["span_noise_per_mille"]),
    (dict(T5, span_noise_per_mille=-5), ARG, ["span_noise_per_mille"]),
    (dict(T5, span_noise_per_mille=501), ARG, ["span_noise_per_mille"]),
    (dict(T5, avg_span_size=0.99), ARG, ["avg_span_size"]),
    (dict(T5, avg_span_size=0.0), ARG, ["avg_span_size"]),
    (dict(T5, avg_span_size=float("inf")), ARG, ["avg_span_size"]),
    (dict(T5, avg_span_size=float("nan")), ARG, ["avg_span_size"]),
    # a full row's labels or sentinels do not fit; the message names the numbers
    (dict(T5, sequence_length=2048), ARG, ["307", "102", "410", "512", "103", "100"]),
    (dict(T5, sequence_length=512, span_noise_per_mille=200, avg_span_size=3.0), ARG, ["102", "34", "137", "128"]),
    (dict(T5, sequence_length=64, span_noise_per_mille=500, avg_span_size=3.0), ARG, ["32", "11", "44", "16"]),
    (dict(T5, rng_mode=1), UNSUPPORTED, ["span_policy", "rng_mode"]),
])
def test_create_refuses_before_it_looks_for_a_device(native_lib, fields, code, words):
    """SDL_ERR_ARG (-1) / SDL_ERR_UNSUPPORTED (-4) with or without a GPU, never SDL_ERR_NODEV.
    Code that ignores the two words answers 0 or SDL_ERR_NODEV to every one of these."""
    rc, msg = create_rc(native_lib, **fields)
    assert rc == code, (rc, msg)
    assert all(w in msg for w in words), msg


@pytest.mark.parametrize("fields", [
    dict(T5), dict(T5, sequence_length=64), dict(T5, sequence_length=2048, span_noise_per_mille=100),
    dict(T5, span_noise_per_mille=1), dict(T5, avg_span_size=1.0, span_noise_per_mille=100),
    dict(T5, avg_span_gap=-3.0),                                # ignored under policy 1
    dict(span_policy=0, span_noise_per_mille=0),                # zeroed words: today's config
    dict(span_policy=0, span_noise_per_mille=900, avg_span_size=0.2),  # ... whose other words nobody reads
])
def test_create_accepts_what_the_contract_accepts(native_lib, fields):
    """No argument error: the call gets as far as the device (0 with one, SDL_ERR_NODEV without)."""
    rc, msg = create_rc(native_lib, **fields)
    assert rc in (0, -5), (rc, msg)


def test_capacity_bound_is_the_models(native_lib):
    """Around the bound at S = 512, mean 3.0: create refuses exactly where the model's full row
    needs more than S/4 labels or 100 sentinels."""
    for pm in range(170, 200):
        need, sent = M.capacity(512, pm, 3.0)
        rc, msg = create_rc(native_lib, **dict(T5, span_noise_per_mille=pm))
        assert (rc == ARG) == (need > 128 or sent > 100), (pm, need, sent, rc, msg)


# ---- span_noise.hpp on the host ---------------------------------------------------------------------------
def test_span_noise_header_under_sanitizers(tmp_path):
    exe = str(tmp_path / "span_noise_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "span_noise_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "span_noise ok" in r.stdout


def test_model_counts_equal_the_headers(tmp_path):
    """The model's (t, m) against span_noise_counts for every n up to 2048 (one double step each side)."""
    src = tmp_path / "counts.cpp"
    src.write_text('#include <cstdio>\n#include "span_noise.hpp"\nint main() {\n'
                   '  const int pm[] = {1, 50, 100, 150, 172, 300, 500}; const double mean[] = {1.0, 1.5, 2.0, 3.0, 5.5, 50.0};\n'
                   '  for (int p : pm) for (double q : mean) for (int n = 0; n <= 2048; ++n) {\n'
                   '    int t, m; sdl::span_noise_counts(n, p, q, &t, &m); std::printf("%d %d\\n", t, m); }\n  return 0; }\n')
    exe = str(tmp_path / "counts")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", exe], check=True)
    got = np.array(subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split(), int).reshape(-1, 2)
    want = [M.counts(n, p, q) for p in (1, 50, 100, 150, 172, 300, 500) for q in (1.0, 1.5, 2.0, 3.0, 5.5, 50.0)
            for n in range(2049)]
    assert got.tolist() == [list(w) for w in want]
