"""csrc/list_index.hpp -- id index -> (chunk, position in the chunk's list) and the record's chunk
bracket, as the rows kernel and the row map use them -- against a brute-force walk, in a
stand-alone host program (tests/list_index_check.cpp) built with the host compiler's address and
undefined-behaviour sanitizers.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "streaming_data_loader_amd", "csrc")


def host_compiler():
    for c in (os.environ.get("CXX"), "g++", "clang++", "c++"):
        if c and shutil.which(c):
            return shutil.which(c)
    pytest.fail("no host C++ compiler found")


def test_list_index_against_brute_force(tmp_path):
    exe = str(tmp_path / "list_index_check")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "list_index_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "list_index ok" in r.stdout
