"""sdl_best_fit / sdl_batcher_set_best_fit without a device: the struct's size and field offsets from
ctypes and from a C compiler over the header, and the two declarations in INTEGRATION.md's FFI block."""
import ctypes
import os
import shutil
import subprocess

import pytest

from streaming_data_loader_amd import native

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sdl_best_fit_layout(tmp_path):
    assert ctypes.sizeof(native.BestFit) == 16
    assert [getattr(native.BestFit, f).offset for f in ("window_records", "reserved")] == [0, 4]
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "bf.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sdl_batcher.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(sdl_best_fit), offsetof(sdl_best_fit, window_records),\n'
                   '         offsetof(sdl_best_fit, reserved));\n  return 0;\n}\n')
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), str(src), "-o", str(tmp_path / "bf")], check=True)
    out = subprocess.run([str(tmp_path / "bf")], capture_output=True, text=True, check=True).stdout
    assert [int(x) for x in out.split()] == [16, 0, 4]


def test_ffi_declarations_are_documented():
    with open(os.path.join(REPO, "INTEGRATION.md"), encoding="utf-8") as f:
        doc = f.read()
    assert "#[repr(C)] pub struct SdlBestFit {" in doc
    assert "pub fn sdl_batcher_set_best_fit(h: *mut SdlBatcher, bf: *const SdlBestFit) -> c_int;" in doc
    assert "sdl_batcher_set_best_fit" in native.EXPORTS
