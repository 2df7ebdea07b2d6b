"""sdl_zstd_inflate_device on the GPU against the committed fixtures (tests/golden/zstd, made once
with libzstd and the pure-Python writer; no libzstd is needed here): every fixture alone and all of
them in one call are bit-exact, corrupt frames between good ones are refused with their status while
the good ones still decode, the checksum flag, the provider chain .zst -> JsonText -> records, and
the reference-exact call (the first frame's range only).  The corrupt list is the one the host model
handles under the sanitizers in tests/test_zstd_format.py."""
import numpy as np
import pytest

import zstd_cases as zc

pytestmark = pytest.mark.gpu

MAN = zc.load_manifest()["fixtures"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def db(native_lib):
    from streaming_data_loader_amd.device import DeviceBatcher
    return DeviceBatcher(batch_size=8, sequence_length=128)


@pytest.fixture(scope="module")
def plains():
    return {e["name"]: zc.fixture_plain(e) for e in MAN}


def device_zstd(torch, db, buf, offsets, flags=0):
    """One call over buf with the frame ranges `offsets` -> (rc, Inflated, status[n], per-frame bytes, arena)."""
    from streaming_data_loader_amd import native
    n = len(offsets) - 1
    off = np.asarray(offsets, np.uint64)
    a = np.zeros(len(buf) + 32, np.uint8)
    a[:len(buf)] = np.frombuffer(buf, np.uint8)
    d_z = torch.from_numpy(a).cuda()
    d_off = torch.from_numpy(off.view(np.int64)).cuda()
    rc, out = db.zstd_inflate(d_z.data_ptr(), len(buf), d_off.data_ptr(), n, flags=flags, check=False)
    assert rc in (0, native.SDL_ERR_DATA), native.load().sdl_last_error()
    assert out.n_members == n
    status = np.zeros(n, np.int32)
    mo = np.zeros(n + 1, np.uint32)
    arena = np.zeros(int(out.out_bytes) + 32, np.uint8)
    if n:
        native.d2h(db._h, status, out.d_status, status.nbytes)
    native.d2h(db._h, mo, out.d_member_out, mo.nbytes)
    native.d2h(db._h, arena, out.d_out, arena.nbytes)
    assert out.d_out % 16 == 0
    assert mo[0] == 0 and mo[n] == out.out_bytes and (np.diff(mo.astype(np.int64)) >= 0).all()
    assert (arena[int(out.out_bytes):] == 0).all()  # 32 zero bytes after
    assert out.n_bad == int((status != 0).sum())
    assert (rc == 0) == (out.n_bad == 0)
    return rc, out, status, [arena[int(mo[i]):int(mo[i + 1])].tobytes() for i in range(n)], arena


def frame_plains(z, plain, offsets):
    """The plaintext of each frame of a fixture file (one frame: all of it; the skippable mix: from the writer)."""
    frames = zc.walk(z)
    real = [i for i, f in enumerate(frames) if "skippable" not in f["modes"]]
    if len(real) == 1:
        return [plain if i == real[0] else b"" for i in range(len(frames))]
    parts = {n: p for n, _z, p, _e in zc.written_frames()}
    pa, pb = parts["w_rle_literals"], parts["w_rle_then_repeat"]
    assert plain == pa + pb and len(real) == 2
    return [pa if i == real[0] else pb if i == real[1] else b"" for i in range(len(frames))]


@pytest.mark.parametrize("entry", MAN, ids=[e["name"] for e in MAN])
def test_every_fixture_alone(torch, db, plains, entry):
    from streaming_data_loader_amd import native
    z = zc.fixture_bytes(entry)
    off = native.zstd_split_frames(z)
    rc, out, status, got, arena = device_zstd(torch, db, z, off)
    assert rc == 0 and (status == 0).all(), status
    assert arena[:int(out.out_bytes)].tobytes() == plains[entry["name"]]
    assert got == frame_plains(z, plains[entry["name"]], off)


def all_in_one(plains):
    """Every fixture as one call, skippable frames among them: (buffer, offsets, expected bytes per frame)."""
    buf, off, want = b"", [0], []

    def add(z, frames):
        nonlocal buf
        base = len(buf)
        buf += z
        off.extend(base + o for o in zc.split(z)[1:])
        want.extend(frames)

    add(zc.skippable(b"first"), [b""])
    for i, e in enumerate(MAN):
        z = zc.fixture_bytes(e)
        add(z, frame_plains(z, plains[e["name"]], zc.split(z)))
        if i % 4 == 3:
            add(zc.skippable(bytes(i), i & 15), [b""])
    add(zc.skippable(b""), [b""])
    return buf, off, want


def test_all_fixtures_in_one_call_and_again(torch, db, plains):
    buf, off, want = all_in_one(plains)
    assert 36 <= len(want) <= 48
    rc, out, status, got, arena = device_zstd(torch, db, buf, off)
    assert rc == 0 and (status == 0).all(), status
    for i, (g, w) in enumerate(zip(got, want)):  # d_member_out for every frame
        assert g == w, i
    assert out.out_bytes == sum(len(w) for w in want)
    rc2, out2, status2, got2, arena2 = device_zstd(torch, db, buf, off)
    assert rc2 == 0 and (arena2 == arena).all() and (status2 == status).all()
    # a small call after the large one reads none of its buffers
    e = next(e for e in MAN if e["name"] == "w_repeat_offsets")
    z = zc.fixture_bytes(e)
    rc3, out3, status3, got3, _ = device_zstd(torch, db, z, [0, len(z)])
    assert rc3 == 0 and got3 == [plains["w_repeat_offsets"]]
    rc4, out4, _, got4, _ = device_zstd(torch, db, b"", [0])
    assert rc4 == 0 and out4.out_bytes == 0 and got4 == []


def test_corrupt_frames_between_good_ones(torch, db, plains):
    from streaming_data_loader_amd import native
    good_a = zc.fixture_bytes(next(e for e in MAN if e["name"] == "small3000_sum"))
    good_b = zc.fixture_bytes(next(e for e in MAN if e["name"] == "w_repeat_offsets"))
    buf, off, kinds = b"", [0], []
    cases = zc.corrupt_cases()
    for name, z, want in cases:
        for part, kind in ((good_a, "a"), (z, (name, want)), (good_b, "b")):
            buf += part
            off.append(len(buf))
            kinds.append(kind)
    rc, out, status, got, _ = device_zstd(torch, db, buf, off)
    assert rc == native.SDL_ERR_DATA and out.n_bad == len(cases)
    msg = native.load().sdl_last_error().decode()
    assert "zstd frame 1:" in msg and f"{len(cases)} of {len(kinds)} frames failed" in msg, msg
    for i, kind in enumerate(kinds):
        if kind == "a":
            assert status[i] == 0 and got[i] == plains["small3000_sum"], i
        elif kind == "b":
            assert status[i] == 0 and got[i] == plains["w_repeat_offsets"], i
        else:
            name, want = kind
            assert status[i] != 0, name
            if want is not None:
                assert status[i] == want, (name, status[i])


def test_no_checksum_flag_accepts_the_bad_checksum_only(torch, db, plains):
    from streaming_data_loader_amd import native
    cases = zc.corrupt_cases()
    buf, off = b"", [0]
    for _name, z, _want in cases:
        buf += z
        off.append(len(buf))
    rc, out, status, got, _ = device_zstd(torch, db, buf, off, flags=native.SDL_ZSTD_NO_CHECKSUM)
    ok = [name for (name, _, _), s in zip(cases, status) if s == 0]
    assert ok == ["bad_checksum"] and rc == native.SDL_ERR_DATA
    i = [name for name, _, _ in cases].index("bad_checksum")
    assert got[i] == plains["small3000_sum"]
    rc, out, status, got, _ = device_zstd(torch, db, cases[i][1], [0, len(cases[i][1])])
    assert rc == native.SDL_ERR_DATA and status[0] == native.ZS_E_CHECKSUM


def test_provider_chain_zst_to_records(torch, db, records):
    """records.jsonl.zst -> zstd_inflate -> json_text: the records the provider sends."""
    from streaming_data_loader_amd import native
    z = zc.fixture_bytes(next(e for e in MAN if e["name"] == "records_sum"))
    rc, out, status, got, _ = device_zstd(torch, db, z, native.zstd_split_frames(z))
    assert rc == 0
    jt = db.json_text(out.d_out, int(out.out_bytes))
    offs = np.zeros(jt.n_records + 1, np.uint64)
    native.d2h(db._h, offs, jt.d_offsets, offs.nbytes)
    text = np.zeros(int(jt.text_bytes), np.uint8)
    native.d2h(db._h, text, jt.d_text, text.nbytes)
    assert [text[int(offs[i]):int(offs[i + 1])].tobytes().decode() for i in range(jt.n_records)] == records


def test_reference_exact_call_takes_the_first_frame(torch, db, plains):
    """async-compression's decoder with multiple_members off stops after the first frame: the call
    that passes only the first non-skippable frame's range yields that frame's lines."""
    from streaming_data_loader_amd import native
    first = zc.fixture_bytes(next(e for e in MAN if e["name"] == "heldout_70k"))
    second = zc.fixture_bytes(next(e for e in MAN if e["name"] == "records_sum"))
    file = zc.skippable(b"index") + first + second
    off = native.zstd_split_frames(file)
    frames = zc.walk(file)
    k = next(i for i, f in enumerate(frames) if "skippable" not in f["modes"])
    assert k == 1
    rc, out, status, got, _ = device_zstd(torch, db, file, [int(off[k]), int(off[k + 1])])
    assert rc == 0 and got == [plains["heldout_70k"]]
    assert got[0].endswith(b"\n") or b"\n" in got[0]
