"""sdl_fim / sdl_batcher_set_fim without a device: the struct's size and field offsets from ctypes
and from a C compiler over the header, and the two declarations in INTEGRATION.md's FFI block (which
tests/test_integration_ffi.py then compares with the header field by field)."""
import ctypes
import os
import shutil
import subprocess

import pytest

from streaming_data_loader_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["rate_per_mille", "spm_per_mille", "prefix_id", "suffix_id", "middle_id", "reserved"]


def test_sdl_fim_layout(tmp_path):
    assert ctypes.sizeof(native.Fim) == 32
    assert [getattr(native.Fim, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "fim.c"
    offs = ", ".join(f"offsetof(sdl_fim, {f})" for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdl_batcher.h"\nint main(void) {\n'
                   f'  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sdl_fim), {offs});\n  return 0;\n}}\n')
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "fim")], check=True)
    out = subprocess.run([str(tmp_path / "fim")], capture_output=True, text=True, check=True).stdout
    assert [int(x) for x in out.split()] == [32, 0, 4, 8, 12, 16, 20]


def test_ffi_declarations_are_documented():
    with open(os.path.join(REPO, "INTEGRATION.md"), encoding="utf-8") as f:
        doc = f.read()
    assert "#[repr(C)] pub struct SdlFim {" in doc
    assert "pub fn sdl_batcher_set_fim(h: *mut SdlBatcher, fim: *const SdlFim) -> c_int;" in doc
    assert "sdl_batcher_set_fim" in native.EXPORTS
