"""Packed span rows (sdl_config.pack = 1 under the span task): the chunk length and what
sdl_batcher_create decides from the config and the tokenizer alone, with or without a GPU."""
import ctypes

import pytest

import pack_span_model as model
from streaming_data_loader_amd import native

# (S, per mille, mean) -> N of the contract's table (None: refused)
TABLE = [(512, 150, 3.0, 569), (64, 150, 3.0, 71), (128, 150, 3.0, 142), (1024, 150, 3.0, 1138), (33, 100, 3.0, 36),
         (33, 150, 3.0, None), (2048, 120, 3.0, 2226), (2048, 150, 3.0, None), (64, 1, 3.0, 64)]
GRID = [(S, pm, mean) for S, pm, mean, _ in TABLE] + [(S, pm, mean) for S in (64, 512, 2048) for pm in (1, 150, 500)
                                                      for mean in (1.0, 7.3)]


def config(S, per_mille, mean, **kw):
    c = native.default_config(native.SDL_TASK_SPAN)
    c.pack, c.span_policy, c.sequence_length = 1, 1, S
    c.span_noise_per_mille, c.avg_span_size = per_mille, mean
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def create(native_lib, c, tokenizer=native.T5_PROXY_TOKENIZER):
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), tokenizer.encode(), native.DATA_DIR.encode(), ctypes.byref(h))
    if h.value:
        native_lib.sdl_batcher_destroy(h)
    return rc, native_lib.sdl_last_error()


@pytest.mark.parametrize("S,per_mille,mean,N", TABLE)
def test_the_contracts_table(S, per_mille, mean, N):
    assert model.chunk_length(S, per_mille, mean) == N


@pytest.mark.parametrize("S,per_mille,mean", GRID)
def test_chunk_length_equals_the_model(native_lib, S, per_mille, mean):
    want = model.chunk_length(S, per_mille, mean)
    got = native_lib.sdl_pack_span_length(ctypes.byref(config(S, per_mille, mean)))
    if want is None:
        assert got == -1 and b"pack" in native_lib.sdl_last_error()  # SDL_ERR_ARG
    else:
        assert got == want >= S


@pytest.mark.parametrize("S", [33, 2048])
def test_refused_before_the_device_check(native_lib, S):
    rc, msg = create(native_lib, config(S, 150, 3.0))
    assert rc == -1 and b"pack" in msg and (b"labels" in msg)


def test_accepted_config_passes_the_argument_checks(native_lib):
    rc, _ = create(native_lib, config(64, 150, 3.0, batch_size=4))
    assert rc in (0, -5)  # created, or SDL_ERR_NODEV on a machine without a GPU


def test_a_bert_tokenizer_is_refused(native_lib):
    rc, msg = create(native_lib, config(64, 150, 3.0, batch_size=4), native.BERT_PROXY_TOKENIZER)
    assert rc == -4 and b"pack" in msg and b"Unigram" in msg  # SDL_ERR_UNSUPPORTED
