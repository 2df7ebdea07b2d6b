"""Packed clm rows (sdl_config.pack = 1), the parts that need no GPU: the numpy model of the
contract (tests/pack_model.py) on a hand-written example, the config word through the ctypes and
Python layers, the refusals sdl_batcher_create makes before it looks for a device, and the host
queue's bookkeeping (csrc/pack_queue.hpp) in a stand-alone program under the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pack_model
from streaming_data_loader_amd import batcher as B
from streaming_data_loader_amd import native

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "streaming_data_loader_amd", "csrc")
E = 9  # the example's eos


def test_model_on_a_hand_written_example():
    # S = 4.  Documents: [1 2 3 4 5], [] (dropped: no ids), [6], [7 8] -> the stream
    #   1 2 3 4 | 5 E 6 E | 7 8 E      with document starts at 0, 6, 8
    ids, am, lab, pos, carry = pack_model.pack([[1, 2, 3, 4, 5], [], [6], [7, 8]], 4, E)
    np.testing.assert_array_equal(ids, [[1, 2, 3, 4], [5, E, 6, E]])
    np.testing.assert_array_equal(lab, ids)
    np.testing.assert_array_equal(am, [[1, 1, 1, 1], [1, 1, 1, 1]])
    # row 1 opens inside document 0 (it began in row 0: positions restart at the row start)
    np.testing.assert_array_equal(pos, [[0, 1, 2, 3], [0, 1, 0, 1]])
    np.testing.assert_array_equal(carry[0], [7, 8, E])
    np.testing.assert_array_equal(carry[1], [0, 1, 2])
    # the next call: the carry in front, [E E] is a document holding the literal eos id twice
    ids, am, lab, pos, carry = pack_model.pack([[E, E], [1, 2, 3]], 4, E, carry=carry)
    np.testing.assert_array_equal(ids, [[7, 8, E, E], [E, E, 1, 2]])
    np.testing.assert_array_equal(pos, [[0, 1, 2, 0], [0, 1, 0, 1]])
    np.testing.assert_array_equal(carry[0], [3, E])
    np.testing.assert_array_equal(carry[1], [0, 1])  # document [1 2 3] goes on: the row restarts it at 0
    # a call that emits no row keeps the carry in front with its positions
    ids, am, lab, pos, carry = pack_model.pack([[4]], 4, E, carry=carry)
    assert ids.shape == (1, 4) and carry[0].size == 0
    np.testing.assert_array_equal(ids, [[3, E, 4, E]])
    np.testing.assert_array_equal(pos, [[0, 1, 0, 1]])
    ids, am, lab, pos, carry = pack_model.pack([[5]], 4, E, carry=carry)
    assert ids.shape == (0, 4)
    ids, am, lab, pos, carry = pack_model.pack([], 4, E, carry=carry)
    assert ids.shape == (0, 4)
    np.testing.assert_array_equal(carry[0], [5, E])
    np.testing.assert_array_equal(carry[1], [0, 1])
    # flush: the plain orientation
    ids, am, lab, pos = pack_model.flush(carry, 4)
    np.testing.assert_array_equal(ids, [[5, E, 0, 0]])
    np.testing.assert_array_equal(am, [[1, 1, 0, 0]])
    np.testing.assert_array_equal(lab, [[5, E, -100, -100]])
    np.testing.assert_array_equal(pos, [[0, 1, 0, 0]])
    assert pack_model.flush(pack_model.EMPTY, 4)[0].shape == (0, 4)


def test_min_ids_filters_on_the_framed_count():
    docs = [[1], [1, 2], [1, 2, 3], []]
    np.testing.assert_array_equal(pack_model.record_rows(docs, 0), [2, 3, 4, 0])
    np.testing.assert_array_equal(pack_model.record_rows(docs, 3), [0, 3, 4, 0])  # n + 1 >= 3
    ids, _, _, _, carry = pack_model.pack(docs, 8, E, min_ids=3)
    np.testing.assert_array_equal(np.concatenate([ids.ravel(), carry[0]]), [1, 2, E, 1, 2, 3, E])


@pytest.mark.parametrize("S", [3, 4, 7, 64])
def test_unpadding_gives_back_the_stream(S):
    rng = np.random.default_rng(S)
    docs = [rng.integers(10, 99, int(n)).tolist() for n in rng.integers(0, 3 * S, 60)]
    docs[5] = [E, 11, E]  # the literal eos id inside a document
    rows, carry = [], pack_model.EMPTY
    for a in range(0, 60, 7):  # several calls, the carry between them
        ids, am, lab, pos, carry = pack_model.pack(docs[a:a + 7], S, E, carry=carry)
        assert (am == 1).all() and (lab == ids).all()
        rows.append((ids, am, pos))
    f = pack_model.flush(carry, S)
    rows.append((f[0], f[1], f[3]))
    ids, am, pos = (np.concatenate([r[k] for r in rows]) for k in range(3))
    want = [t + [E] for t in docs if t]
    assert ids[am == 1].tolist() == [x for t in want for x in t]
    # the pieces position_ids cut the rows into are the documents, cut again at row ends
    pieces = pack_model.unpad(ids, am, pos)
    k = 0
    for t in want:
        got = []
        while len(got) < len(t):
            got += pieces[k].tolist()
            k += 1
        assert got == t
    assert k == len(pieces)
    # position_ids count up inside a piece and never reach S
    for r in range(ids.shape[0]):
        for c in range(1, S):
            if am[r, c]:
                assert pos[r, c] in (0, pos[r, c - 1] + 1)
    assert pos.max() < S and (pos[:, 0] == 0).all()


def test_config_has_pack_and_keeps_its_size():
    assert ctypes.sizeof(native.Config) == 96
    # the word after mask_per_mille, the first of the four that were reserved (the ctypes mirror
    # keeps its four-word `reserved` view over them: reserved[0] is pack)
    assert native.Config.pack.offset == 80 and native.Config.pack.size == 4
    assert native.Config.reserved.offset == 80 and native.Config.reserved.size == 16
    c = native.Config()
    c.pack = 1
    assert list(c.reserved) == [1, 0, 0, 0]


def test_config_pack_is_where_the_header_puts_it(tmp_path):
    """offsetof(sdl_config, pack) and the three reserved words behind it, from a C compiler."""
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc, "no C compiler found"
    src = tmp_path / "pack_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdl_batcher.h"\n'
                   'int main(void) { sdl_config c; printf("%zu %zu %zu %zu\\n", sizeof(sdl_config), '
                   'offsetof(sdl_config, pack), offsetof(sdl_config, reserved), sizeof(c.reserved)); return 0; }\n')
    exe = tmp_path / "pack_layout"
    subprocess.run([cc, "-I", os.path.join(os.path.dirname(HERE), "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(native.Config), native.Config.pack.offset, 84, 12]


def test_native_config_sets_pack(native_lib):
    c, kind = B._native_config(B.BatchConfig(4, 64), B.Gpt(pack=True), True, 0, 0, 0, 0)
    assert (c.pack, c.task, kind) == (1, native.SDL_TASK_CLM, "gpt2")
    c, _ = B._native_config(B.BatchConfig(4, 64), B.Gpt(), True, 0, 0, 0, 0)
    assert c.pack == 0
    assert native.default_config(native.SDL_TASK_CLM).pack == 0


def test_dataset_dict_has_position_ids_only_when_present():
    z = np.zeros((1, 2), np.int32)
    assert set(B.DataSet("gpt2", 1, z, z, z).to_dict()) == {"input_ids", "attention_mask", "labels"}
    assert set(B.DataSet("gpt2", 1, z, z, z, position_ids=z).to_dict()) == {"input_ids", "attention_mask", "labels",
                                                                             "position_ids"}


@pytest.mark.parametrize("task,pack", [(native.SDL_TASK_CLM, 2), (native.SDL_TASK_CLM, -1), (native.SDL_TASK_MLM, 1),
                                       (native.SDL_TASK_SPAN, 1)])
def test_create_refuses_before_the_device_check(native_lib, task, pack):
    """A bad pack word is an argument error with or without a GPU (without the check the call gets
    as far as the device count and answers SDL_ERR_NODEV here)."""
    c = native.default_config(task)
    c.pack = pack
    tok = {native.SDL_TASK_CLM: native.GPT2_PROXY_TOKENIZER, native.SDL_TASK_MLM: native.BERT_PROXY_TOKENIZER,
           native.SDL_TASK_SPAN: native.T5_PROXY_TOKENIZER}[task]
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), tok.encode(), native.DATA_DIR.encode(), ctypes.byref(h))
    assert rc == -1 and not h.value  # SDL_ERR_ARG
    assert b"pack" in native_lib.sdl_last_error()


def test_position_accessors_take_null(native_lib):
    assert not native_lib.sdl_batch_position_ids(None)
    assert not native_lib.sdl_batch_position_ids(ctypes.byref(native.Batch()))
    assert not native_lib.sdl_device_position_ids(None)


def test_pack_queue_bookkeeping_under_sanitizers(tmp_path):
    cxx = next((shutil.which(c) for c in (os.environ.get("CXX"), "g++", "clang++", "c++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "pack_queue_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "pack_queue_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pack_queue ok" in r.stdout
