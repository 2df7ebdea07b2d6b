"""Packed mlm rows (sdl_config.pack = 1 under the MLM task): what sdl_batcher_create decides from the
config alone, with or without a GPU, and one hand-written example of the model."""
import ctypes

import numpy as np
import pytest

import mlm_policy_model as M
import pack_mlm_model
import pack_model
from streaming_data_loader_amd import native


def create(native_lib, **kw):
    c = native.default_config(native.SDL_TASK_MLM)
    c.pack, c.mask_policy = 1, 1
    for k, v in kw.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), native.BERT_PROXY_TOKENIZER.encode(), native.DATA_DIR.encode(),
                                       ctypes.byref(h))
    if h.value:
        native_lib.sdl_batcher_destroy(h)
    return rc, native_lib.sdl_last_error()


@pytest.mark.parametrize("policy", [1, 2])
def test_config_passes_the_argument_checks(native_lib, policy):
    rc, _ = create(native_lib, mask_policy=policy)
    assert rc in (0, -5)  # created, or SDL_ERR_NODEV on a machine without a GPU


@pytest.mark.parametrize("kw,code", [({"rng_mode": 1}, -4), ({"pair": 2}, -1), ({"sequence_length": 2}, -1),
                                     ({"sequence_length": 4096}, -1)])
def test_refused_before_the_device_check(native_lib, kw, code):
    rc, msg = create(native_lib, **kw)
    assert rc == code and b"pack" in msg


def test_model_by_hand():
    """[CLS] 5 6 [SEP] | [CLS] 7 [SEP] at S = 4, nothing masked: one row, the second document carried."""
    _, _, cls, sep = M.proxy_vocab()
    planes, carry = pack_mlm_model.pack([[5, 6], [], [7]], 4, 0, pack_model.EMPTY, 0, 1, seed=3, mask_length=0)
    assert planes.tolist() == [[[cls, 5, 6, sep]], [[1, 1, 1, 1]], [[0, 0, 0, 0]], [[-100] * 4], [[0, 1, 2, 3]]]
    assert carry[0].tolist() == [cls, 7, sep] and carry[1].tolist() == [0, 1, 2]
    fl = pack_mlm_model.flush(carry, 4, 1, 1, seed=3, mask_length=0)
    assert fl[:, 0].tolist() == [[cls, 7, sep, 0], [1, 1, 1, 0], [0] * 4, [-100] * 4, [0, 1, 2, 0]]
    np.testing.assert_array_equal(pack_mlm_model.record_rows([[5, 6], [], [7]], 4), [4, 0, 0])
