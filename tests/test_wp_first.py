"""csrc/wp_first.hpp -- the 16-byte-slot table of the vocabulary's first pieces that the WordPiece
chunk kernel's first probes read (slot layout, hash, the two slot indices, the compare, the cuckoo
build with its seeds) -- in a stand-alone host program (tests/wp_first_check.cpp) built with the
host compiler's address and undefined-behaviour sanitizers.  The program builds the table over
the pieces of assets/bert_proxy/tokenizer.json the way assets.cpp does and checks that every
non-"##" piece of at most 14 bytes is found with its last id, and that no "##" payload, no longer
piece cut to 14 bytes, no piece with one byte changed, added or dropped and none of 100,000 random
lower-case strings is found unless it is such a piece itself; then the same over two synthetic
vocabularies (duplicates and a 14-byte piece that prefixes a 15-byte one; only [UNK] short enough
for the table).  Nothing is loaded into Python."""
import json
import os
import subprocess

from test_list_index import CSRC, HERE, host_compiler

TOKENIZER = os.path.join(os.path.dirname(CSRC), "assets", "bert_proxy", "tokenizer.json")


def test_wp_first_table_finds_exactly_its_pieces(tmp_path):
    with open(TOKENIZER, encoding="utf-8") as f:
        vocab = json.load(f)["model"]["vocab"]
    pieces = [""] * (max(vocab.values()) + 1)
    for piece, i in vocab.items():
        assert "\n" not in piece and "\r" not in piece and not pieces[i]
        pieces[i] = piece
    first = [p for p in pieces if p and not (len(p) > 2 and p.startswith("##"))]
    assert len(pieces) > 30000 and sum(len(p.encode()) <= 14 for p in first) > 20000
    assert max(len(p.encode()) for p in first) >= 15  # (some piece is cut to 14 bytes)
    path = tmp_path / "pieces.txt"
    path.write_bytes("".join(p + "\n" for p in pieces).encode("utf-8"))

    exe = str(tmp_path / "wp_first_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "wp_first_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wp_first ok" in r.stdout
