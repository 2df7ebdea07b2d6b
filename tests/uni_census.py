"""A census of what k_unigram_chunks is handed, chunk by chunk (test infrastructure).

The Unigram chunk kernel (streaming_data_loader_amd/csrc/tokenize_unigram.hip) settles a word on
one of several paths, each with a capacity and a slower fallback that has to give the same ids.
A parity test that never reaches a fallback proves nothing about it, so
tests/test_gpu_unigram_paths.py asserts, before it runs the device, that its input sits on the
side of the limit it says.  This module restates the kernel's *classification* of the words
that start in each 1 KiB chunk -- never its output:

  added      an added token ("<...>", matched on the raw text)
  narrow     a simple word (printable ASCII 0x21..0x7E) of <= UNI_WMAX bytes that the word table
             does not hold: one narrow Viterbi job, one 16-byte payload unit
  wide       a simple word of UNI_WMAX+1 .. UNI_VMAX bytes, when the vocabulary lets the wide
             Viterbi run (wide_ok): one wide job, ceil(L / 16) payload units
  medium     any other word of <= UNI_WMAX bytes (normalized in the chunk's LDS arena)
  long       everything else, and every word whose end the chunk's window does not show
             (word_len reports 0): finished by k_unigram_long / k_unigram_huge

The counts are what the chunk *asks for*; comparing them with UNI_VPC (jobs, and payload
units), MED_CAP and ARENA / UNI_WMAX (medium words) and PFX_JOBS (wide jobs a pass) says
whether a fallback has to run.  Which word of an overfull chunk loses is lane order and is not
modelled.  The constants are read from the sources (constants()), so the census follows a
retune; tests/test_uni_census.py fails when a name disappears.

Word-table membership is decided the way assets.cpp builds the table, for the two cases the
tests use: "▁w" is a piece (a hit), or w is such a piece plus "," or "." (a hit).  The table
also holds other punctuated and capitalised spellings; `clear_miss` therefore only vouches for
words of lower-case letters whose "▁w" is no piece, which no such rule produces.
"""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "streaming_data_loader_amd", "csrc")
NAMES = ("CHUNK", "HALO_L", "HALO_R", "UNI_WMAX", "UNI_VMAX", "UNI_VPC", "UNI_VRING", "MED_CAP", "ARENA",
         "PFX_JOBS", "LONG_NORM1", "LONG_NORM", "LONG_RAW")
META = "▁"
ASCII_WS = (32, 9, 10, 12, 13)  # uni_ascii's U_WS (0x0B is a word byte)


def constants():
    """{name: int} of NAMES, from `constexpr int NAME = <integer>;` in common.hpp and
    tokenize_unigram.hip.  KeyError-free: a missing or non-literal name raises ValueError."""
    text = ""
    for f in ("common.hpp", "tokenize_unigram.hip"):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            text += fh.read()
    out = {}
    for n in NAMES:
        m = re.findall(r"constexpr\s+int\s+(?:\w+\s*=\s*[^,;]+,\s*)*?" + n + r"\s*=\s*(\d+)\s*[;,]", text)
        if len(m) != 1:
            raise ValueError(f"constant {n}: {len(m)} integer definitions found")
        out[n] = int(m[0])
    return out


class Census:
    def __init__(self, vocab, consts=None):
        """vocab: the tokenizer.json model's [piece, score] list (added tokens: "<...>" entries
        at ids 0..2 and 32000.., as the t5 layout has them)."""
        self.K = consts or constants()
        pieces = [p for p, _ in vocab]
        self.added = {p.encode() for i, p in enumerate(pieces)
                      if (i < 3 or i >= 32000) and p.startswith("<") and p.endswith(">")}
        self.max_added = max(map(len, self.added)) if self.added else 0
        ordinary = [p for i, p in enumerate(pieces) if not (i < 3 or i >= 32000)]
        self.base = {p[1:] for p in ordinary if p.startswith(META) and len(p) > 1 and
                     all(0x21 <= ord(c) <= 0x7E for c in p[1:])}
        self.maxlen_first = max(len(p.encode()) for p in ordinary if not p.startswith(META))
        self.maxlen_meta = max(len(p[1:].encode()) for p in ordinary if p.startswith(META))
        self.wide_ok = self.maxlen_first < self.K["UNI_VRING"] and self.maxlen_meta + 3 < self.K["UNI_VRING"]

    def in_word_table(self, w):
        return w in self.base or (len(w) <= self.K["UNI_WMAX"] and w[-1:] in (",", ".") and w[:-1] in self.base)

    def clear_miss(self, w):
        """True for a word no word-table rule can produce."""
        return w.isascii() and w.isalpha() and w.islower() and w not in self.base

    def _added_at(self, b, p, rec_end):
        """Length of the added token starting at p (not crossing the record's end), or 0."""
        if b[p] != 0x3C:
            return 0
        for k in range(1, self.max_added):
            if p + k >= rec_end:
                return 0
            if b[p + k] == 0x3E:
                return k + 1 if bytes(b[p:p + k + 1]) in self.added else 0
        return 0

    def words(self, arena, offs):
        """(start, end, kind) of every piece of the arena in order; kind "added" or "word".
        Words are the runs between ASCII whitespace, record edges and added tokens."""
        b = bytes(arena)
        out = []
        for r in range(len(offs) - 1):
            p, re_ = int(offs[r]), int(offs[r + 1])
            while p < re_:
                if b[p] in ASCII_WS:
                    p += 1
                    continue
                l = self._added_at(b, p, re_)
                if l:
                    out.append((p, p + l, "added"))
                    p += l
                    continue
                e = p + 1
                while e < re_ and b[e] not in ASCII_WS and not self._added_at(b, e, re_):
                    e += 1
                out.append((p, e, "word"))
                p = e
        return out

    def chunks(self, arena, offs):
        """Per 1 KiB chunk of arena[:offs[-1]]: a dict of the counts its words ask for --
        added, hits, narrow (jobs), wide (jobs), units (payload units of narrow + wide),
        medium, long -- and `wide_lens`, the wide jobs' lengths in text order."""
        K = self.K
        N = int(offs[-1])
        b = bytes(arena[:N])
        n_chunks = (N + K["CHUNK"] - 1) // K["CHUNK"]
        out = [dict(added=0, hits=0, narrow=0, wide=0, units=0, medium=0, long=0, wide_lens=[])
               for _ in range(n_chunks)]
        for p, e, kind in self.words(b, offs):
            c = out[p // K["CHUNK"]]
            if kind == "added":
                c["added"] += 1
                continue
            c0 = (p // K["CHUNK"]) * K["CHUNK"]
            L = e - p
            # word_len: the end has to show before the last 8 bytes of the window
            seen = e - c0 < K["CHUNK"] + K["HALO_R"] - 8
            simple = all(0x21 <= x <= 0x7E for x in b[p:e])
            if not seen or L > K["UNI_VMAX"]:
                c["long"] += 1
            elif L <= K["UNI_WMAX"] and simple:
                if self.in_word_table(b[p:e].decode("ascii")):
                    c["hits"] += 1
                else:
                    c["narrow"] += 1
                    c["units"] += 1
            elif L <= K["UNI_WMAX"]:
                c["medium"] += 1
            elif simple and self.wide_ok:
                c["wide"] += 1
                c["units"] += (L + 15) // 16
                c["wide_lens"].append(L)
            else:
                c["long"] += 1
        return out
