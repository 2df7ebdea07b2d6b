"""csrc/wp_pack.hpp -- the mask arithmetic of the WordPiece chunk kernel's id compaction (valid
slot mask -> packed list positions, record boundary -> id offset, a finished piece's exception
bits) -- against naive loops over the stage slots, in a stand-alone host program
(tests/wp_pack_check.cpp) built with the host compiler's address and undefined-behaviour
sanitizers.  Random chunks plus: empty, all 16 bits set in every lane, only tail slots, and
boundaries at offsets 0, 15, 16 and 1023.  Nothing is loaded into Python."""
import os
import subprocess

from test_list_index import CSRC, HERE, host_compiler


def test_wp_pack_against_naive_loops(tmp_path):
    exe = str(tmp_path / "wp_pack_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "wp_pack_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wp_pack ok" in r.stdout
