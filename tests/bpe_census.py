"""A census of what k_bpe_chunks does with its input, chunk by chunk (test infrastructure).

The BPE chunk kernel (streaming_data_loader_amd/csrc/tokenize_bpe.hip) settles every pre-token
that starts in its 1 KiB chunk on one of six paths:

  hit          one probe of the word table finds it (a vocabulary string that encodes to itself;
               17..64 bytes: the bytes past 16 compared with the pool)
  lane         a miss of 2..LANE_BPE bytes: bpe_lane, one word per lane
  wave         a miss of LANE_BPE+1..BPE_MAX_WAVE bytes: bpe_wave_seg, consecutive such misses
               packed into one wave's lanes while their total stays <= 64
  long_lds     longer than BPE_MAX_WAVE, at most LONG_LDS bytes: k_bpe_long in LDS
  long_global  longer than LONG_LDS: k_bpe_long on the global scratch
  past         the chunk's last piece when its end does not show in the window: no pre-token or
               record start in [c1, c1 + HALO_R - 8) (the kernel's `wi < WIN - 8` loop); listed
               with len == 0, its end found by bpe_piece_end, then merged by k_bpe_long in the
               form its length selects (`form`: "lds" or "global")

tests/test_gpu_bpe_paths.py asserts, before it runs the device, that its input sits on the side
of the limit it says; this module restates the kernel's *classification* and never its merging:
the ids come from the caller's `encode` (the plain model of tests/bpe_merge_model.py).  The
constants are read from the sources (constants()), so the census follows a retune;
tests/test_bpe_census.py fails when a name disappears.

Inputs are restricted so that pre-token boundaries are known by construction (`" "? letters+`):
records of letters (ASCII letters and the bytes of multi-byte letters) joined by single spaces; a
record may start with one space and may end with one (`\\s+(?!\\S)` makes that space a piece).
Anything else raises ValueError.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "streaming_data_loader_amd", "csrc")
NAMES = ("CHUNK", "HALO_L", "HALO_R", "WIN", "STAGE", "BPE_MAX_WAVE", "LANE_BPE", "LONG_LDS")
PATHS = ("hit", "lane", "wave", "long_lds", "long_global", "past")


def constants():
    """{name: int} of NAMES from `constexpr int NAME = <expr>;` in common.hpp and
    tokenize_bpe.hip; an expression may use + - * / ( ) over integers and names defined before it.
    A missing name, or one defined twice or by anything else, raises ValueError."""
    text = ""
    for f in ("common.hpp", "tokenize_bpe.hip"):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            text += fh.read()
    known = {}
    for m in re.finditer(r"constexpr\s+int\s+(\w+)\s*=\s*([^;{]+);", text):
        name, expr = m.group(1), m.group(2).strip()
        if not re.fullmatch(r"[\w\s+\-*/()]+", expr):
            continue
        toks = re.findall(r"[A-Za-z_]\w*", expr)
        if any(t not in known for t in toks):
            continue
        val = eval(re.sub(r"/", "//", expr), {"__builtins__": {}}, dict(known))  # integers and known names only
        if name in NAMES and name in known:
            raise ValueError(f"constant {name}: defined twice")
        known[name] = int(val)
    for n in NAMES:
        if n not in known:
            raise ValueError(f"constant {n}: no integer definition found")
    return {n: known[n] for n in NAMES}


def _is_letter(b):
    return 0x61 <= (b | 0x20) <= 0x7A or b >= 0x80


class Census:
    def __init__(self, is_self, encode, consts=None):
        """is_self(piece bytes) -> bool: the piece is a word-table entry; encode(piece bytes) ->
        ids: the reference model's ids of one pre-token."""
        self.K = consts or constants()
        self.is_self = is_self
        self.encode = encode

    def pieces(self, arena, offs):
        """(start, end) of every pre-token of the arena, in order."""
        b = bytes(arena)
        out = []
        for r in range(len(offs) - 1):
            p, re_ = int(offs[r]), int(offs[r + 1])
            while p < re_:
                e = p
                if b[e] == 0x20:
                    e += 1
                    if e == re_:  # the record's trailing space
                        out.append((p, e))
                        break
                if not _is_letter(b[e]):
                    raise ValueError(f"byte {e}: not a letter or a single space")
                while e < re_ and _is_letter(b[e]):
                    e += 1
                out.append((p, e))
                p = e
        return out

    def chunks(self, arena, offs):
        """Per 1 KiB chunk of arena[:offs[-1]] a dict: `pieces` [(start, length, path)] of the
        pre-tokens starting in it (path in PATHS), `form` {start: "lds" | "global"} of its long
        and past-window pieces, `packs` (the wave path's packings: lists of lengths), `entries`
        (list entries the chunk kernel writes: a long piece is one marker) and `ids` (after
        k_bpe_long's fix-up)."""
        K = self.K
        N = int(offs[-1])
        b = bytes(arena[:N])
        n_chunks = (N + K["CHUNK"] - 1) // K["CHUNK"]
        out = [dict(pieces=[], form={}, packs=[], entries=0, ids=0) for _ in range(n_chunks)]
        ps = self.pieces(b, offs)
        for i, (p, e) in enumerate(ps):
            ci = p // K["CHUNK"]
            c0 = ci * K["CHUNK"]
            c = out[ci]
            n = e - p
            last = i + 1 == len(ps) or ps[i + 1][0] // K["CHUNK"] != ci
            seen = not last or e - c0 < K["CHUNK"] + K["HALO_R"] - 8
            k = len(self.encode(b[p:e]))
            if not seen or n > K["BPE_MAX_WAVE"]:
                path = "past" if not seen else "long_lds" if n <= K["LONG_LDS"] else "long_global"
                c["form"][p] = "lds" if n <= K["LONG_LDS"] else "global"
                c["entries"] += 1
            else:
                path = "hit" if self.is_self(b[p:e]) else "lane" if n <= K["LANE_BPE"] else "wave"
                assert path != "lane" or n >= 2  # (a single byte symbol is always a table entry)
                c["entries"] += k
            c["ids"] += k
            c["pieces"].append((p, n, path))
        for c in out:
            total, pack = 0, []
            for _, n, path in c["pieces"]:
                if path != "wave":
                    continue
                if total + n > 64:
                    c["packs"].append(pack)
                    total, pack = 0, []
                pack.append(n)
                total += n
            if pack:
                c["packs"].append(pack)
        return out


def count_paths(chunks, into=None):
    """{path: pieces} over a census, added to `into`; past-window pieces also count under
    "past/lds" or "past/global", long ones as their path says."""
    acc = into if into is not None else {}
    for c in chunks:
        for p, _, path in c["pieces"]:
            acc[path] = acc.get(path, 0) + 1
            if path == "past":
                k = "past/" + c["form"][p]
                acc[k] = acc.get(k, 0) + 1
    return acc
