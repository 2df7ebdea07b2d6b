"""The Zstandard format code (csrc/zstd_format.hpp) on the CPU, before any kernel runs it: the
committed fixtures cover every mode of the format the decoder handles; the hand-written frames are
legal (libzstd decodes them); sdl_zstd_split_frames agrees with the pure-Python header walker; and
the host model (tests/zstd_host_model.cpp -- the same parsers, table builders, bit reader, symbolic
repeat offsets and XXH64 the kernels use, stage by stage) decodes every fixture to its plaintext and
gives every corrupt case a non-zero status, as a stand-alone program built with the host compiler's
address and undefined-behaviour sanitizers.  Nothing sanitized is loaded into Python."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import zstd_cases as zc
from test_list_index import CSRC, HERE, host_compiler

MAN = zc.load_manifest()["fixtures"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zsmodel") / "zstd_host_model")
    cmd = [host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(HERE, "zstd_host_model.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    return exe


def run_model(exe, paths, outdir=None, flags=()):
    cmd = [exe, *flags] + (["--outdir", str(outdir)] if outdir else []) + [str(p) for p in paths]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr
    out = {}
    for line in r.stdout.splitlines():
        m = re.match(r"(\S+) status=(\d+) frames=(\d+) bad=(\d+) out=(\d+) xxh64=(\w+) rep=([\d,]+) fstatus=([\d,]*)$", line)
        assert m, line
        out[os.path.basename(m.group(1))] = {
            "status": int(m.group(2)), "frames": int(m.group(3)), "bad": int(m.group(4)), "out": int(m.group(5)),
            "rep": [int(x) for x in m.group(7).split(",")], "fstatus": [int(x) for x in m.group(8).split(",") if x]}
    return out


def test_fixture_files_match_the_manifest():
    files = sorted(f for f in os.listdir(zc.ZDIR) if f.endswith(".zst"))
    assert files == sorted(e["file"] for e in MAN)
    assert sum(os.path.getsize(os.path.join(zc.ZDIR, f)) for f in files) < 2 << 20
    for e in MAN:
        z = zc.fixture_bytes(e)
        assert len(z) < 400 << 10
        assert sorted(zc.modes_of(z)) == e["modes"], e["name"]  # re-walked from the bytes
        plain = zc.fixture_plain(e)
        assert len(plain) == e["plain_len"] and zc.sha256(plain) == e["sha256"], e["name"]


def test_fixtures_cover_every_mode(model):
    have = set()
    for e in MAN:
        have |= zc.modes_of(zc.fixture_bytes(e)) | set(e["extra"]) - set(zc.REP_NAMES)
    res = run_model(model, [os.path.join(zc.ZDIR, e["file"]) for e in MAN])
    for r in res.values():
        have |= {name for name, count in zip(zc.REP_NAMES, r["rep"]) if count}
    assert not zc.REQUIRED_MODES - have, sorted(zc.REQUIRED_MODES - have)


def test_written_frames_are_legal_zstd():
    libs = zc.find_libzstd()
    if not libs:
        pytest.skip("no libzstd on this machine")
    for lib in libs:
        for name, z, plain, _extra in zc.written_frames():
            assert lib.decompress(z, len(plain)) == plain, (lib.version, name)
        # (the corrupt cases really are corrupt: libzstd refuses them too, but for three the format
        # forbids and some libzstd versions let pass)
        lenient = {"repeat_offset_zero", "flip_seq_modes_reserved", "block_over_max"}
        for name, z, want in zc.corrupt_cases():
            assert lib.decompress(z, 4 << 20) is None or name in lenient, (lib.version, name)


def many_frame_files():
    z = {e["name"]: zc.fixture_bytes(e) for e in MAN}
    yield b""
    yield z["tiny40"] + zc.skippable(b"") + z["small3000_sum"]
    yield zc.skippable(b"abc", 3) + z["empty"] + z["heldout_l9_flush4k"] + zc.skippable(bytes(1000), 15) + z["run300k"]
    yield b"".join(z[k] for k in sorted(z))


def test_split_frames_equals_the_walker(native_lib):
    from streaming_data_loader_amd import native
    for e in MAN:
        z = zc.fixture_bytes(e)
        assert list(native.zstd_split_frames(z)) == zc.split(z), e["name"]
    for z in many_frame_files():
        assert list(native.zstd_split_frames(z)) == zc.split(z)
    # truncated inputs, and bytes that are no frame: SDL_ERR_DATA, as the walker raises
    z = zc.fixture_bytes(MAN[0]) + next(zc.fixture_bytes(e) for e in MAN if e["name"] == "small3000_sum")
    for cut in (1, 3, 4, 5, 8, len(z) // 2, len(z) - 5, len(z) - 1):
        with pytest.raises(zc.BadFrame):
            zc.split(z[:cut])
        with pytest.raises(native.SDLError) as ei:
            native.zstd_split_frames(z[:cut])
        assert ei.value.code == native.SDL_ERR_DATA
    for name, bad, _want in zc.corrupt_cases():
        try:
            want = zc.split(bad)
        except zc.BadFrame:
            with pytest.raises(native.SDLError) as ei:
                native.zstd_split_frames(bad)
            assert ei.value.code == native.SDL_ERR_DATA, name
        else:
            assert list(native.zstd_split_frames(bad)) == want, name
    # a too-small cap: SDL_ERR_CAPACITY with the count set
    import ctypes
    z = list(many_frame_files())[2]
    n = ctypes.c_uint64(0)
    off = np.zeros(3, np.uint64)
    assert native_lib.sdl_zstd_split_frames(z, len(z), off.ctypes.data, 3, ctypes.byref(n)) == -7
    assert n.value == len(zc.split(z)) - 1 == 5
    assert native_lib.sdl_zstd_split_frames(z, len(z), None, 0, ctypes.byref(n)) == -7 and n.value == 5


def test_host_model_decodes_every_fixture(model, tmp_path):
    res = run_model(model, [os.path.join(zc.ZDIR, e["file"]) for e in MAN], outdir=tmp_path)
    for e in MAN:
        r = res[e["file"]]
        assert r["status"] == 0 and r["bad"] == 0 and r["out"] == e["plain_len"], (e["name"], r)
        with open(tmp_path / (e["file"] + ".out"), "rb") as f:
            assert hashlib.sha256(f.read()).hexdigest() == e["sha256"], e["name"]
    # concatenations, skippable frames among them, as one file
    for i, z in enumerate(many_frame_files()):
        p = tmp_path / f"many{i}.zst"
        p.write_bytes(z)
        r = run_model(model, [p], outdir=tmp_path)[p.name]
        assert r["status"] == 0 and r["frames"] == len(zc.split(z)) - 1
        lib = (zc.find_libzstd() or [None])[0]
        if lib:
            assert (tmp_path / (p.name + ".out")).read_bytes() == lib.decompress(z, 8 << 20)


def test_host_model_refuses_every_corrupt_case(model, tmp_path):
    cases = zc.corrupt_cases()
    for name, z, _want in cases:
        (tmp_path / (name + ".zst")).write_bytes(z)
    res = run_model(model, [tmp_path / (name + ".zst") for name, _, _ in cases])
    for name, _z, want in cases:
        r = res[name + ".zst"]
        assert r["status"] != 0, name
        if want is not None:
            assert r["status"] == want, (name, r)
    # the checksum flag accepts the bad-checksum frame and nothing else
    res = run_model(model, [tmp_path / (name + ".zst") for name, _, _ in cases], flags=["--no-checksum"])
    assert sorted(n for n, _, _ in cases if res[n + ".zst"]["status"] == 0) == ["bad_checksum"]
