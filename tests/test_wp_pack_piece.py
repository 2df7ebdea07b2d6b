"""The WordPiece chunk list taken by piece, against a naive walk over the stage slots, in a
stand-alone host program (tests/wp_pack_piece_check.cpp) built with the host compiler's address
and undefined-behaviour sanitizers: the gather of an exception-free chunk through its piece
descriptors (csrc/wp_pack.hpp wp_pair_slots, stale descriptors included) and the kernel's test
for such a chunk; and, as arithmetic only -- the kernel packs a chunk with exceptions slot by slot
-- a piece's list position from its lane's {base, valid mask} record and its shift D against the
piece number.  4,000 random chunks (piece starts, ids up to a piece's bytes, pieces without an
id, tail slots) plus: empty, one piece, 1,024 one-byte pieces, an exception in slot 0, 15, 16 and
1023, two exceptions in one 16-slot group, and a last word whose ids reach the tail slots.
Nothing is loaded into Python."""
import os
import subprocess

from test_list_index import CSRC, HERE, host_compiler


def test_wp_pack_by_piece_against_naive_walk(tmp_path):
    exe = str(tmp_path / "wp_pack_piece_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "wp_pack_piece_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wp_pack_piece ok" in r.stdout
