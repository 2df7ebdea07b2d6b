"""csrc/wp_extent.hpp -- the word extents of the WordPiece chunk kernel's first probes (stop and
fast-terminator bits of 16 bytes, a word's length and fast flag from the two bitmaps, the keep
mask and the one-OR lower-casing) -- against a byte-wise restatement of the rule word_setup used
before the bitmaps, in a stand-alone host program (tests/wp_extent_check.cpp) built with the host
compiler's address and undefined-behaviour sanitizers.  Every piece start of random windows over
a weighted byte alphabet with random record starts, text ends and non-ASCII bits, plus: words of
15, 16, 17 and 33 bytes, a record start at p, p + 1, p + 15 and p + 16, words that end at chunk
offsets 1023, 1024, 1039 and 1040, the text ending inside a word, a non-ASCII first byte, a
window of letters and digits only, and empty lanes.  Nothing is loaded into Python."""
import os
import subprocess

from test_list_index import CSRC, HERE, host_compiler


def test_wp_extent_against_bytewise_rule(tmp_path):
    exe = str(tmp_path / "wp_extent_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "wp_extent_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wp_extent ok" in r.stdout
