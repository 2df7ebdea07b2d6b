"""A byte-level BPE tokenizer in RoBERTa's form (post_processor RobertaProcessing): what the host
loader reads from it and refuses, and what sdl_batcher_create decides from the config alone -- with
or without a GPU."""
import ctypes

import pytest

import pack_mlm_bpe_model as model
from streaming_data_loader_amd import native


@pytest.fixture(scope="module")
def tk(tmp_path_factory):
    return model.roberta_tokenizer(tmp_path_factory.mktemp("roberta") / "tokenizer.json")


def test_tokenizer_info(native_lib, tk):
    info = native.tokenizer_info(tk.path)
    assert (info.kind, info.vocab_size, info.eos_id, info.n_added) == (1, 50261, model.SEP, 5)


@pytest.mark.parametrize("edit,names", [({"cls": 17}, "post_processor.cls"), ({"mask_lstrip": True}, "lstrip"),
                                        ({"post": False}, "<|endoftext|>")])
def test_loader_refuses_naming_the_field(native_lib, tmp_path, edit, names):
    bad = model.roberta_tokenizer(tmp_path / "tokenizer.json", **edit)
    with pytest.raises(native.SDLError) as e:
        native.tokenizer_info(bad.path)
    assert e.value.code == -2 and names in str(e.value)  # SDL_ERR_IO


def test_endoftext_stays_the_eos_of_a_file_that_has_one(native_lib, tmp_path):
    both = model.roberta_tokenizer(tmp_path / "tokenizer.json", keep_eot=True, post=False)
    assert native.tokenizer_info(both.path).eos_id == 50256


@pytest.mark.parametrize("kw,code", [({}, (0, -5)), ({"mask_policy": 2}, (0, -5)), ({"mask_policy": 0}, (-1,)),
                                     ({"rng_mode": 1}, (-4,)), ({"pair": 2}, (-1,)), ({"sequence_length": 2}, (-1,)),
                                     ({"sequence_length": 4096}, (-1,))])
def test_create_from_the_config_alone(native_lib, tk, kw, code):
    """Accepted configs reach the device check (created, or SDL_ERR_NODEV); the others are refused before it."""
    c = native.default_config(native.SDL_TASK_MLM)
    c.pack, c.mask_policy, c.mask_id = 1, 1, tk.mask
    for k, v in kw.items():
        setattr(c, k, v)
    h = ctypes.c_void_p()
    rc = native_lib.sdl_batcher_create(ctypes.byref(c), tk.path.encode(), native.DATA_DIR.encode(), ctypes.byref(h))
    if h.value:
        native_lib.sdl_batcher_destroy(h)
    assert rc in code and (rc >= 0 or rc == -5 or b"pack" in native_lib.sdl_last_error())
