"""build.py's SOURCES and HEADERS are the native sources, whole: source_hash() hashes exactly those
files (plus include/sdl_batcher.h), so a file of csrc/ missing from the lists -- or an #include of a
file outside them -- could change without the library's build id noticing, and a stale library
would load as up to date."""
import os
import re

from streaming_data_loader_amd import build as b

ABI_HEADER = os.path.join(b.REPO, "include", "sdl_batcher.h")


def test_lists_are_the_directory():
    listed = b.SOURCES + b.HEADERS
    assert len(listed) == len(set(listed)), "a file is listed twice"
    assert sorted(listed) == sorted(os.listdir(b.CSRC))


def test_every_quoted_include_is_hashed():
    hashed = {os.path.join(b.CSRC, f) for f in b.SOURCES + b.HEADERS} | {ABI_HEADER}
    seen = 0
    for f in b.SOURCES + b.HEADERS:
        with open(os.path.join(b.CSRC, f), encoding="utf-8") as fh:
            for inc in re.findall(r'^\s*#\s*include\s*"([^"]+)"', fh.read(), re.M):
                seen += 1
                assert os.path.normpath(os.path.join(b.CSRC, inc)) in hashed, (f, inc)
    assert seen > 0
