"""Zstandard test material: seeded plaintext recipes, a pure-Python header walker (modes only, no
entropy decode), a pure-Python frame writer for the modes libzstd does not emit, the corrupt-case
list, and a ctypes binding of whatever libzstd the machine has (fixtures are made with it once and
committed; the GPU tests read only the committed files)."""
import ctypes
import ctypes.util
import glob
import hashlib
import json
import os
import random
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
ZDIR = os.path.join(GOLDEN, "zstd")
MANIFEST = os.path.join(ZDIR, "manifest.json")

MAGIC = 0xFD2FB528
# status codes of csrc/zstd_format.hpp (zs::E_*) = kernels.hpp ZS_E_*
(ZS_OK, ZS_E_RANGE, ZS_E_TRUNC, ZS_E_MAGIC, ZS_E_DICT, ZS_E_WINDOW, ZS_E_BTYPE, ZS_E_BSIZE, ZS_E_LITHDR, ZS_E_HUF,
 ZS_E_FSE, ZS_E_SEQHDR, ZS_E_ENDBITS, ZS_E_FAR, ZS_E_SIZE, ZS_E_CHECKSUM, ZS_E_STALL) = range(17)


# ---------------------------------------------------------------------------------------------
# libzstd through ctypes
class _Buf(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("size", ctypes.c_size_t), ("pos", ctypes.c_size_t)]


class LibZstd:
    C_LEVEL, C_WINDOWLOG, C_CONTENTSIZE, C_CHECKSUM = 100, 101, 200, 201

    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        self.path = path
        sz, vp, i = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int
        L.ZSTD_versionString.restype = ctypes.c_char_p
        self.version = L.ZSTD_versionString().decode()
        L.ZSTD_compressBound.restype, L.ZSTD_compressBound.argtypes = sz, [sz]
        L.ZSTD_isError.restype, L.ZSTD_isError.argtypes = ctypes.c_uint, [sz]
        L.ZSTD_createCCtx.restype = vp
        L.ZSTD_freeCCtx.argtypes = [vp]
        L.ZSTD_CCtx_setParameter.restype, L.ZSTD_CCtx_setParameter.argtypes = sz, [vp, i, i]
        L.ZSTD_compress2.restype, L.ZSTD_compress2.argtypes = sz, [vp, vp, sz, ctypes.c_char_p, sz]
        L.ZSTD_compressStream2.restype = sz
        L.ZSTD_compressStream2.argtypes = [vp, ctypes.POINTER(_Buf), ctypes.POINTER(_Buf), i]
        L.ZSTD_decompress.restype, L.ZSTD_decompress.argtypes = sz, [vp, sz, ctypes.c_char_p, sz]

    def _cctx(self, level, checksum, content_size, window_log):
        c = self.L.ZSTD_createCCtx()
        for k, v in ((self.C_LEVEL, level), (self.C_CHECKSUM, int(checksum)), (self.C_CONTENTSIZE, int(content_size))):
            assert not self.L.ZSTD_isError(self.L.ZSTD_CCtx_setParameter(c, k, v))
        if window_log:
            assert not self.L.ZSTD_isError(self.L.ZSTD_CCtx_setParameter(c, self.C_WINDOWLOG, window_log))
        return c

    def compress(self, data, level=3, checksum=False, content_size=True, window_log=0):
        c = self._cctx(level, checksum, content_size, window_log)
        cap = self.L.ZSTD_compressBound(len(data))
        dst = ctypes.create_string_buffer(cap)
        n = self.L.ZSTD_compress2(c, dst, cap, data, len(data))
        self.L.ZSTD_freeCCtx(c)
        assert not self.L.ZSTD_isError(n)
        return dst.raw[:n]

    def stream(self, data, level=3, flush_every=4096, checksum=False, window_log=0):
        """Streaming compression (no content size) with a flush every `flush_every` input bytes."""
        c = self._cctx(level, checksum, True, window_log)
        cap = self.L.ZSTD_compressBound(len(data)) + 16 * (len(data) // flush_every + 2) + 64
        dst = ctypes.create_string_buffer(cap)
        src = ctypes.create_string_buffer(data, len(data) or 1)
        ob = _Buf(ctypes.addressof(dst), cap, 0)
        pos = 0
        while True:
            end = min(len(data), pos + flush_every)
            ib = _Buf(ctypes.addressof(src), end, pos)
            last = end == len(data)
            while True:
                r = self.L.ZSTD_compressStream2(c, ctypes.byref(ob), ctypes.byref(ib), 2 if last else 1)
                assert not self.L.ZSTD_isError(r)
                if r == 0:
                    break
            pos = end
            if last:
                break
        self.L.ZSTD_freeCCtx(c)
        return dst.raw[:ob.pos]

    def decompress(self, z, cap):
        """Every frame of z (ZSTD_decompress takes concatenated and skippable frames); None on error."""
        dst = ctypes.create_string_buffer(cap + 1)
        n = self.L.ZSTD_decompress(dst, cap + 1, z, len(z))
        return None if self.L.ZSTD_isError(n) else dst.raw[:n]


def find_libzstd():
    """Every distinct libzstd on this machine, as [LibZstd], oldest version first."""
    cands = []
    name = ctypes.util.find_library("zstd")
    if name:
        cands.append(name)
    for d in (os.path.join(sys.prefix, "lib"), "/usr/lib/x86_64-linux-gnu", "/usr/lib64", "/usr/lib"):
        cands += sorted(glob.glob(os.path.join(d, "libzstd.so.1")))
    try:
        import PIL
        cands += sorted(glob.glob(os.path.join(os.path.dirname(os.path.dirname(PIL.__file__)), "pillow.libs", "libzstd*")))
    except Exception:
        pass
    libs, seen = [], set()
    for c in cands:
        try:
            lib = LibZstd(c)
        except (OSError, AttributeError):
            continue
        if lib.version not in seen:
            seen.add(lib.version)
            libs.append(lib)
    return sorted(libs, key=lambda x: [int(t) for t in x.version.split(".")])


# ---------------------------------------------------------------------------------------------
# plaintext recipes (seeded; the slices are of the committed JSON-lines fixtures)
def _golden(name):
    with open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read()


def plaintext(recipe):
    kind = recipe["plain"]
    n = recipe.get("n", 0)
    r = random.Random(recipe.get("seed", 1))
    if kind == "empty":
        return b""
    if kind == "random":
        return bytes(r.getrandbits(8) for _ in range(n))
    if kind == "run":
        return b"a" * n
    if kind == "digits":
        return bytes(r.choice(b"0123456789") for _ in range(n))
    if kind == "skewed":
        return bytes(r.choice(b"aaaaaaaabbbbccd ") for _ in range(n))
    if kind == "heldout":
        return _golden("heldout_records.jsonl")[:n or None]
    if kind == "records":
        return _golden("test_records.jsonl")[:n or None]
    raise ValueError(kind)


# name, plaintext recipe, encoder settings
LIB_RECIPES = [
    ("empty", {"plain": "empty"}, {}),
    ("empty_sum", {"plain": "empty"}, {"checksum": True}),
    ("tiny40", {"plain": "heldout", "n": 40}, {}),
    ("skewed200", {"plain": "skewed", "n": 200}, {}),
    ("small3000_sum", {"plain": "heldout", "n": 3000}, {"checksum": True}),
    ("random200k", {"plain": "random", "n": 200000}, {}),
    ("run300k", {"plain": "run", "n": 300000}, {"checksum": True}),
    ("digits300k", {"plain": "digits", "n": 300000}, {}),
    ("records_flush2k", {"plain": "records"}, {"flush_every": 2048}),
    ("records_sum", {"plain": "records"}, {"checksum": True}),
    ("heldout_l3", {"plain": "heldout", "n": 1000000}, {"checksum": True}),
    ("heldout_l1", {"plain": "heldout", "n": 1000000}, {"level": 1}),
    ("heldout_neg5", {"plain": "heldout", "n": 400000}, {"level": -5}),
    ("heldout_l9_flush4k", {"plain": "heldout", "n": 300000}, {"level": 9, "flush_every": 4096, "checksum": True}),
    ("heldout_w17", {"plain": "heldout", "n": 500000}, {"window_log": 17, "content_size": False}),
    ("heldout_w19_stream", {"plain": "heldout", "n": 500000}, {"window_log": 19, "flush_every": 1 << 20}),
    ("heldout_w21_l19", {"plain": "heldout", "n": 250000}, {"level": 19, "window_log": 21, "checksum": True}),
    ("heldout_70k", {"plain": "heldout", "n": 70000}, {}),
]


# made again with the newest libzstd found, when it is another version (name + "_new")
NEWER_RECIPES = ("heldout_l9_flush4k",)


def lib_compress(lib, plain, enc):
    if "flush_every" in enc:
        return lib.stream(plain, enc.get("level", 3), enc["flush_every"], enc.get("checksum", False), enc.get("window_log", 0))
    return lib.compress(plain, enc.get("level", 3), enc.get("checksum", False), enc.get("content_size", True),
                        enc.get("window_log", 0))


# ---------------------------------------------------------------------------------------------
# the walker: frame, block and section headers only
class BadFrame(ValueError):
    pass


def _frame_header(z, a):
    if a + 4 > len(z):
        raise BadFrame("truncated magic")
    magic = struct.unpack_from("<I", z, a)[0]
    if magic & 0xFFFFFFF0 == 0x184D2A50:
        if a + 8 > len(z):
            raise BadFrame("truncated skippable header")
        return {"skippable": True, "hdr": 8, "size": struct.unpack_from("<I", z, a + 4)[0]}
    if magic != MAGIC:
        raise BadFrame("bad magic")
    if a + 5 > len(z):
        raise BadFrame("truncated header")
    fhd = z[a + 4]
    fcs_flag, single, did_flag = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    if fhd & 8:
        raise BadFrame("reserved bit")
    did_b = 4 if did_flag == 3 else did_flag
    fcs_b = single if fcs_flag == 0 else 1 << fcs_flag
    hdr = 5 + (0 if single else 1) + did_b + fcs_b
    if a + hdr > len(z):
        raise BadFrame("truncated header")
    q = a + 5
    window = None
    wlog = None
    if not single:
        wlog = 10 + (z[q] >> 3)
        if wlog > 31:
            raise BadFrame("window log over the supported limit")
        window = (1 << wlog) + ((1 << wlog) >> 3) * (z[q] & 7)
        q += 1
    did = int.from_bytes(z[q:q + did_b], "little")
    q += did_b
    fcs = int.from_bytes(z[q:q + fcs_b], "little") + (256 if fcs_b == 2 else 0) if fcs_b else None
    if single:
        window = fcs
    return {"skippable": False, "hdr": hdr, "single": bool(single), "wlog": wlog, "window": window, "did": did,
            "fcs": fcs, "fcs_bytes": fcs_b, "checksum": bool(fhd & 4)}


def _compressed_block_modes(b, modes, info):
    """Section headers of one compressed block's content b."""
    b0 = b[0]
    t, sf = b0 & 3, (b0 >> 2) & 3
    if t < 2:
        hdr = 1 if not sf & 1 else (2 if sf == 1 else 3)
        regen = int.from_bytes(b[:hdr], "little") >> (3 if hdr == 1 else 4)
        content = regen if t == 0 else 1
        modes.add("lit_rle" if t else f"lit_raw_h{hdr}")
    else:
        hdr = 3 if sf < 2 else sf + 2
        v = int.from_bytes(b[:hdr], "little") >> 4
        bits = {3: 10, 4: 14, 5: 18}[hdr]
        regen, content = v & ((1 << bits) - 1), v >> bits
        streams = 1 if sf == 0 else 4
        modes.add(f"lit_huf_{streams}s_h{hdr}")
        if t == 3:
            modes.add("lit_treeless")
        else:
            modes.add(("huf_weights_fse_" if b[hdr] < 128 else "huf_weights_direct_") + f"{streams}s")
    info["lit"] = (0, hdr, hdr + content)
    q = hdr + content
    n0 = b[q]
    if n0 == 0:
        modes.add("nseq_0")
        info["seq"] = (q, q + 1)
        return
    nb = 1 if n0 < 128 else (2 if n0 < 255 else 3)
    modes.add(f"nseq_{nb}b")
    m = b[q + nb]
    for name, mode in (("ll", m >> 6), ("of", (m >> 4) & 3), ("ml", (m >> 2) & 3)):
        modes.add(f"{name}_{('predef', 'rle', 'fse', 'repeat')[mode]}")
    info["seq"] = (q, q + nb + 1)


def walk(z):
    """[{'start', 'end', 'modes': set, 'blocks': [{'hdr': offset, 'type', 'size', 'lit', 'seq'}], ...}] for the
    frames of z; raises BadFrame on bytes that are no frame (bad magic, truncation, block type 3)."""
    frames = []
    a = 0
    while a < len(z):
        h = _frame_header(z, a)
        modes = set()
        fr = {"start": a, "modes": modes, "blocks": [], "header": h}
        if h["skippable"]:
            end = a + 8 + h["size"]
            if end > len(z):
                raise BadFrame("truncated skippable frame")
            modes.add("skippable")
        else:
            if h["did"]:
                modes.add("dict_id")
            modes.add("checksum" if h["checksum"] else "no_checksum")
            if h["fcs"] is None:
                modes.add("no_fcs")
            elif h["single"]:
                modes.add(f"single_fcs{h['fcs_bytes']}")
            else:
                modes.add(f"windowed_fcs{h['fcs_bytes']}")
            if not h["single"]:
                modes.add(f"window_{h['wlog']}")
            if h["fcs_bytes"] == 8:
                modes.add("fcs8")
            bmax = min(h["window"], 128 << 10)
            q = a + h["hdr"]
            while True:
                if q + 3 > len(z):
                    raise BadFrame("truncated block header")
                bh = int.from_bytes(z[q:q + 3], "little")
                last, bt, bs = bh & 1, (bh >> 1) & 3, bh >> 3
                if bt == 3:
                    raise BadFrame("block type 3")
                if bs > bmax:
                    raise BadFrame("block over the maximum size")
                content = 1 if bt == 1 else bs
                if q + 3 + content > len(z):
                    raise BadFrame("truncated block")
                info = {"hdr": q, "type": bt, "size": bs, "content": (q + 3, q + 3 + content)}
                modes.add(("block_raw", "block_rle", "block_compressed")[bt])
                if bt == 2:
                    try:
                        _compressed_block_modes(z[q + 3:q + 3 + content], modes, info)
                    except (IndexError, KeyError):
                        pass  # a damaged section: the frame's extent is still known
                fr["blocks"].append(info)
                q += 3 + content
                if last:
                    break
            if h["checksum"]:
                if q + 4 > len(z):
                    raise BadFrame("truncated checksum")
                q += 4
            end = q
            if h["fcs"] == 0 and len(fr["blocks"]) == 1 and fr["blocks"][0]["size"] == 0:
                modes.add("empty_frame")
        fr["end"] = end
        frames.append(fr)
        a = end
    return frames


def split(z):
    """Frame offsets [n + 1] of z (what sdl_zstd_split_frames returns)."""
    return [0] + [f["end"] for f in walk(z)]


def modes_of(z):
    out = set()
    for f in walk(z):
        out |= f["modes"]
    return out


# ---------------------------------------------------------------------------------------------
# the writer: legal frames with the modes libzstd does not emit
class BackWriter:
    """A bitstream the decoder reads backward: write the fields in reverse read order."""

    def __init__(self):
        self.v, self.n = 0, 0

    def add(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0
        self.v |= value << self.n
        self.n += bits

    def finish(self):
        v = self.v | 1 << self.n
        return v.to_bytes((self.n + 8) // 8, "little")


def frame_header(fcs=None, fcs_bytes=None, single=False, window_log=None, checksum=False, dict_id=None, reserved=False):
    if fcs_bytes is None:
        fcs_bytes = 0 if fcs is None else (1 if single and fcs < 256 else 2 if 256 <= fcs < 65536 + 256 else 4 if fcs < 1 << 32 else 8)
    flag = {0: 0, 1: 0, 2: 1, 4: 2, 8: 3}[fcs_bytes]
    assert fcs_bytes != 1 or single
    did_b = 0 if dict_id is None else 4
    fhd = flag << 6 | int(single) << 5 | int(reserved) << 3 | int(checksum) << 2 | (3 if did_b else 0)
    out = struct.pack("<IB", MAGIC, fhd)
    if not single:
        out += bytes([(window_log - 10) << 3])
    if did_b:
        out += struct.pack("<I", dict_id)
    if fcs_bytes:
        out += (fcs - (256 if fcs_bytes == 2 else 0)).to_bytes(fcs_bytes, "little")
    return out


def block(kind, content, last=False, size=None):
    """kind 0 raw, 1 RLE (content = the byte, size = run length), 2 compressed."""
    n = len(content) if size is None else size
    return (int(last) | kind << 1 | n << 3).to_bytes(3, "little") + content


def lit_header_raw(kind, regen, hdr=None):
    hdr = hdr or (1 if regen < 32 else 2 if regen < 4096 else 3)
    if hdr == 1:
        return bytes([kind | regen << 3])
    return (kind | (1 if hdr == 2 else 3) << 2 | regen << 4).to_bytes(hdr, "little")


def literals_raw(data, hdr=None):
    return lit_header_raw(0, len(data), hdr) + data


def literals_rle(byte, regen):
    return lit_header_raw(1, regen) + bytes([byte])


def huf_codes(weights):
    """weights[s] for every symbol (the last one included) -> {s: (code, nbits)} as the decoder's table lays them out."""
    total = sum(1 << (w - 1) for w in weights if w)
    log = total.bit_length() - 1
    assert 1 << log == total
    codes, at = {}, 0
    for w in range(1, log + 1):
        for s, ws in enumerate(weights):
            if ws == w:
                codes[s] = (at >> (w - 1), log + 1 - w)
                at += 1 << (w - 1)
    return codes


def huf_stream(data, codes):
    w = BackWriter()
    for s in reversed(data):
        w.add(*codes[s])
    return w.finish()


def literals_huf_direct(data, weights, streams, treeless=False):
    """Huffman literals with a direct (4-bit) weight list; weights lists every symbol, the last is implied."""
    codes = huf_codes(weights)
    desc = b""
    if not treeless:
        ws = list(weights[:-1])
        desc = bytes([127 + len(ws)]) + bytes((ws[i] << 4) | (ws[i + 1] if i + 1 < len(ws) else 0) for i in range(0, len(ws), 2))
    if streams == 1:
        body = huf_stream(data, codes)
    else:
        seg = (len(data) + 3) // 4
        parts = [huf_stream(data[k * seg:(k + 1) * seg], codes) for k in range(4)]
        body = struct.pack("<HHH", *(len(p) for p in parts[:3])) + b"".join(parts)
    comp, regen = len(desc) + len(body), len(data)
    assert regen < 1024 and comp < 1024
    v = (3 if treeless else 2) | (0 if streams == 1 else 1) << 2 | regen << 4 | comp << 14
    return v.to_bytes(3, "little") + desc + body


LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def nseq_bytes(n, force3=False):
    if n >= 0x7F00 or force3:
        assert n >= 0x7F00
        return bytes([255]) + (n - 0x7F00).to_bytes(2, "little")
    if n < 128:
        return bytes([n])
    return bytes([128 + (n >> 8), n & 255])


def sequences_rle(seqs, ll_code, of_code, ml_code, repeat=False, trailing_bits=0):
    """A sequences section whose three tables are RLE_Mode (or Repeat_Mode of such a block): every sequence
    (ll, ml, offset_value) shares the three codes, the bitstream holds the extra bits only."""
    w = BackWriter()
    w.add(0, trailing_bits)  # (corrupt cases: bits the decoder never reads)
    for ll, ml, ov in reversed(seqs):
        w.add(ll - LL_BASE[ll_code], LL_BITS[ll_code])
        w.add(ml - ML_BASE[ml_code], ML_BITS[ml_code])
        w.add(ov - (1 << of_code), of_code)
    head = nseq_bytes(len(seqs))
    if repeat:
        return head + bytes([0xFC]) + w.finish()
    return head + bytes([0x54, ll_code, of_code, ml_code]) + w.finish()


def run_sequences(literals, seqs, history):
    """What (literals, [(ll, ml, offset)]) regenerates after `history`."""
    out = bytearray(history)
    p = 0
    for ll, ml, off in seqs:
        out += literals[p:p + ll]
        p += ll
        for _ in range(ml):
            out.append(out[-off])
    out += literals[p:]
    return bytes(out[len(history):])


def written_frames():
    """[(name, frame bytes, plaintext, modes the headers do not show)] -- every one legal (libzstd decodes it)."""
    out = []
    lits = bytes(random.Random(7).choice(b"\x00\x01\x02\x03") for _ in range(400))
    w4 = [3, 2, 1, 1]  # symbols 0..3; the last weight is implied

    def frame(name, blocks, plain, extra=(), **hdr):
        hdr.setdefault("window_log", 17)
        body = b"".join(block(*b[:2], last=(i == len(blocks) - 1), **(b[2] if len(b) > 2 else {})) for i, b in enumerate(blocks))
        out.append((name, frame_header(**hdr) + body, plain, sorted(extra)))

    frame("w_rle_literals", [(2, literals_rle(0x41, 50) + b"\x00")], b"A" * 50)
    frame("w_huf_direct_1s", [(2, literals_huf_direct(lits[:100], w4, 1) + b"\x00")], lits[:100])
    frame("w_huf_direct_4s", [(2, literals_huf_direct(lits, w4, 4) + b"\x00")], lits)
    frame("w_treeless_direct", [(2, literals_huf_direct(lits[:90], w4, 1) + b"\x00"),
                                (2, literals_huf_direct(lits[90:], w4, 4, treeless=True) + b"\x00")], lits)
    # RLE_Mode for all three tables, then an all-repeat block (Repeat_Mode for ML too); the second block's
    # first match copies from the first block
    raw = bytes(range(64, 128))
    s1 = [(2, 6, 12 + 3), (2, 6, 10 + 3), (2, 6, 8 + 3)]  # offsets 12, 10, 8 (offset code 3, 3 extra bits)
    l1 = b"abcdefg"
    p1 = run_sequences(l1, [(a, b, c - 3) for a, b, c in s1], raw)
    s2 = [(2, 6, 12 + 3), (2, 6, 6 + 3)]  # offset 12 reaches into block 1, then offset 6
    l2 = b"HIJKLMN"
    p2 = run_sequences(l2, [(a, b, c - 3) for a, b, c in s2], raw + p1)
    frame("w_rle_then_repeat", [(0, raw), (2, literals_raw(l1) + sequences_rle(s1, 2, 3, 3)),
                                (2, literals_raw(l2) + sequences_rle(s2, 2, 3, 3, repeat=True))],
          raw + p1 + p2, extra=["match_from_previous_block"])
    # the 3-byte nbSeq form: 32,512 sequences of ll 1 / ml 3 / offset 1 (an overlapping match)
    n3 = 0x7F00
    l3 = bytes((i * 7) & 0xFF for i in range(n3))
    p3 = b"".join(bytes([c]) * 4 for c in l3)
    frame("w_nseq3_overlap1", [(2, literals_raw(l3) + sequences_rle([(1, 3, 4)] * n3, 1, 2, 0))], p3,
          extra=["overlap_offset_1"], fcs=len(p3), fcs_bytes=8)
    # repeat offsets: Offset_Value 1, 2, 3 with ll > 0 and with ll = 0
    hist = bytes(range(32, 96))
    blocks, plain, reps = [(0, hist)], bytearray(hist), [1, 4, 8]

    def rep_block(ll_code, of_code, seqs):
        lit = bytes(65 + (len(plain) + i) % 26 for i in range(sum(s[0] for s in seqs) + 2))
        real = []
        for ll, ml, ov in seqs:
            idx = ov - 1 + (ll == 0)
            off = reps[0] if idx == 0 else reps[0] - 1 if idx == 3 else reps[idx]
            if idx in (1,):
                reps[0], reps[1] = reps[1], reps[0]
            elif idx:
                reps[:] = [off, reps[0], reps[1]]
            real.append((ll, ml, off))
        blocks.append((2, literals_raw(lit) + sequences_rle(seqs, ll_code, of_code, 0)))
        plain.extend(run_sequences(lit, real, bytes(plain)))

    # seed the history with three distinct offsets through real offsets (offset code 5: values 32 .. 63)
    seed = [(1, 3, 40 + 3), (1, 3, 30 + 3), (1, 3, 35 + 3)]
    lit0 = b"pqrs"
    plain.extend(run_sequences(lit0, [(a, b, c - 3) for a, b, c in seed], bytes(plain)))
    blocks.append((2, literals_raw(lit0) + sequences_rle(seed, 1, 5, 0)))
    reps[:] = [35, 30, 40]
    rep_block(1, 0, [(1, 3, 1), (1, 3, 1)])              # ov 1, ll > 0
    rep_block(1, 1, [(1, 3, 2), (1, 3, 3), (1, 3, 2)])   # ov 2 and 3, ll > 0
    rep_block(0, 0, [(0, 3, 1), (0, 3, 1)])              # ov 1, ll = 0
    rep_block(0, 1, [(0, 3, 2), (0, 3, 3), (0, 3, 3)])   # ov 2 and 3 (rep[0] - 1), ll = 0
    frame("w_repeat_offsets", blocks, bytes(plain), extra=["rep_ov1_ll", "rep_ov2_ll", "rep_ov3_ll", "rep_ov1_ll0",
                                                           "rep_ov2_ll0", "rep_ov3_ll0"], checksum=False)
    # skippable frames before, between and after two frames (one file of five frames)
    (_, za, pa, _), (_, zb, pb, _) = out[0], out[4]
    out.append(("w_skippable_mix", skippable(b"meta") + za + skippable(b"", 7) + zb + skippable(b"x" * 300, 15), pa + pb, []))
    return out


def skippable(payload, nibble=0):
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload)) + payload


# every mode the fixtures must cover between them: the header walker's names, the writer's declared
# extras, and the host model's repeat-offset counts (rep_ov<value>_ll = ll > 0, _ll0 = ll == 0)
REQUIRED_MODES = {
    "block_raw", "block_rle", "block_compressed", "lit_treeless", "lit_huf_1s_h3", "lit_huf_4s_h3", "lit_huf_4s_h4",
    "lit_huf_4s_h5", "lit_raw_h1", "lit_raw_h2", "lit_raw_h3", "huf_weights_fse_1s", "huf_weights_fse_4s",
    "ll_predef", "of_predef", "ml_predef", "ll_fse", "of_fse", "ml_fse", "ll_repeat", "of_repeat", "nseq_1b", "nseq_2b",
    "single_fcs1", "single_fcs2", "single_fcs4", "window_17", "window_19", "window_21", "no_fcs", "checksum",
    "no_checksum", "empty_frame",
    # the modes libzstd does not emit (the writer's frames)
    "lit_rle", "huf_weights_direct_1s", "huf_weights_direct_4s", "ll_rle", "of_rle", "ml_rle", "ml_repeat", "nseq_0",
    "nseq_3b", "skippable", "fcs8", "match_from_previous_block", "overlap_offset_1",
    "rep_ov1_ll", "rep_ov2_ll", "rep_ov3_ll", "rep_ov1_ll0", "rep_ov2_ll0", "rep_ov3_ll0",
}
REP_NAMES = ("rep_ov1_ll", "rep_ov1_ll0", "rep_ov2_ll", "rep_ov2_ll0", "rep_ov3_ll", "rep_ov3_ll0")  # the model's order


# ---------------------------------------------------------------------------------------------
# fixtures as committed
def load_manifest():
    with open(MANIFEST) as f:
        return json.load(f)


def fixture_bytes(entry):
    with open(os.path.join(ZDIR, entry["file"]), "rb") as f:
        return f.read()


def fixture_plain(entry):
    """The plaintext of a fixture: from its recipe (libzstd fixtures) or from the writer (by name)."""
    if entry["recipe"]["plain"] == "written":
        for name, _z, plain, _extra in written_frames():
            if name == entry["name"]:
                return plain
        raise KeyError(entry["name"])
    return plaintext(entry["recipe"])


def sha256(b):
    return hashlib.sha256(b).hexdigest()


# ---------------------------------------------------------------------------------------------
# corrupt cases: (name, bytes, expected status or None where it depends on where a decoder notices)
def corrupt_cases():
    man = {e["name"]: e for e in load_manifest()["fixtures"]}
    cases = []
    multi = fixture_bytes(man["heldout_l9_flush4k"])  # many blocks, checksum, Repeat_Mode tables
    fr = walk(multi)[0]
    cuts = {4: "magic", fr["header"]["hdr"]: "frame_header"}
    for i in (0, 1, len(fr["blocks"]) - 1):
        b = fr["blocks"][i]
        cuts[b["hdr"] + 3] = f"block{i}_header"
        if "lit" in b and "seq" in b:
            c0 = b["content"][0]
            cuts[c0 + b["lit"][1]] = f"block{i}_lit_header"
            cuts[c0 + b["lit"][2]] = f"block{i}_literals"
            cuts[c0 + b["seq"][1]] = f"block{i}_seq_header"
            cuts[b["content"][1] - 1] = f"block{i}_bitstream"
        cuts[b["content"][1]] = f"block{i}_end"
    cuts[len(multi) - 4] = "before_checksum"
    cuts[len(multi) - 1] = "in_checksum"
    for at, what in sorted(cuts.items()):
        if 0 < at < len(multi):
            cases.append((f"trunc_{what}", multi[:at], None))

    def flip(z, at, bit, name, want=None):
        m = bytearray(z)
        m[at] ^= 1 << bit
        cases.append((name, bytes(m), want))

    small = fixture_bytes(man["small3000_sum"])
    sf = walk(small)[0]
    b0 = sf["blocks"][0]
    c0 = b0["content"][0]
    flip(small, 0, 0, "flip_magic", ZS_E_MAGIC)
    flip(small, 4, 3, "reserved_bit", ZS_E_MAGIC)
    flip(small, 4, 0, "dict_id_flag", None)           # one more header byte is read as the id
    flip(small, b0["hdr"], 3, "flip_block_size", None)
    flip(small, c0, 4, "flip_lit_header", None)
    flip(small, c0 + b0["lit"][1] + 1, 0, "flip_huf_desc", None)
    flip(small, c0 + b0["seq"][0], 0, "flip_nseq", None)
    flip(small, c0 + b0["seq"][1] - 1, 1, "flip_seq_modes_reserved", ZS_E_SEQHDR)
    flip(small, b0["content"][1] - 1, 7, "flip_bitstream_end", None)
    flip(small, len(small) - 1, 0, "bad_checksum", ZS_E_CHECKSUM)
    flip(small, c0 + b0["lit"][2] - 1, 7, "flip_literal_stream_end", None)  # the last Huffman stream's end mark
    # a wrong content size (single-segment header: byte 5.. is the size)
    m = bytearray(small)
    assert sf["header"]["single"] and sf["header"]["fcs_bytes"] == 2
    m[5] ^= 1
    cases.append(("wrong_content_size", bytes(m), ZS_E_SIZE))
    raw = bytes(range(64, 128))
    tail = block(0, raw, last=True)
    cases.append(("dictionary_id", frame_header(window_log=17, dict_id=7) + tail, ZS_E_DICT))
    cases.append(("block_type_3", frame_header(window_log=17) + block(3, raw, last=True), ZS_E_BTYPE))
    cases.append(("block_over_max", frame_header(window_log=10) + block(0, bytes(1025), last=True), ZS_E_BSIZE))
    cases.append(("window_log_over_limit", struct.pack("<IBB", MAGIC, 0, (41 - 10) << 3) + tail, ZS_E_WINDOW))

    def one(name, content, want, pre=True):
        blocks = (block(0, raw) if pre else b"") + block(2, content, last=True)
        cases.append((name, frame_header(window_log=17) + blocks, want))

    # an FSE accuracy log over the limit: LL table description whose 4 bits say 15 + 5
    one("accuracy_log_over_limit", literals_raw(b"abcd") + bytes([1, 0x80, 0x0F, 0, 0, 0x01]), ZS_E_FSE)
    # direct Huffman weights 3, 2, 1 + 1, 1: the sum 9 leaves no power of two
    bad_w = bytes([127 + 5, 0x32, 0x11, 0x10])
    body = bytes([0x01, 0x01])
    v = 2 | 0 << 2 | 10 << 4 | (len(bad_w) + len(body)) << 14
    one("huffman_weights_not_power_of_two", v.to_bytes(3, "little") + bad_w + body + b"\x00", ZS_E_HUF)
    one("offset_before_frame_start", literals_raw(b"abcd") + sequences_rle([(1, 3, 200 + 3)], 1, 7, 0), ZS_E_FAR)
    one("offset_before_frame_start_first_block", literals_raw(b"abcd") + sequences_rle([(1, 3, 2 + 3)], 1, 2, 0), ZS_E_FAR,
        pre=False)
    one("repeat_offset_zero", literals_raw(b"abcd") + sequences_rle([(0, 3, 3)], 0, 1, 0), ZS_E_FAR)
    one("repeat_mode_with_nothing_before", literals_raw(b"abcd") + sequences_rle([(1, 3, 4)], 1, 2, 0, repeat=True), ZS_E_SEQHDR)
    lits = bytes([0, 1, 2, 3] * 10)
    one("treeless_with_nothing_before", literals_huf_direct(lits, [3, 2, 1, 1], 1, treeless=True) + b"\x00", ZS_E_HUF)
    one("bitstream_bits_left_over", literals_raw(b"abcd") + sequences_rle([(1, 3, 4)], 1, 2, 0, trailing_bits=3), ZS_E_ENDBITS)
    one("bitstream_no_end_mark", literals_raw(b"abcd") + bytes([1, 0x54, 1, 2, 0, 0x00]), ZS_E_ENDBITS)
    one("literal_lengths_over_literals", literals_raw(b"ab") + sequences_rle([(3, 3, 4)], 3, 2, 0), ZS_E_SEQHDR)
    one("offset_code_over_31", literals_raw(b"abcd") + bytes([1, 0x54, 1, 32, 0, 0x01]), ZS_E_WINDOW)
    one("nseq0_with_trailing_bytes", literals_raw(b"abcd") + b"\x00\x00", ZS_E_SEQHDR)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    return cases
