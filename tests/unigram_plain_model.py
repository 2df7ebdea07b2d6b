"""The plain model of `tokenizers`' Unigram::encode_optimized for one pre-token, with switches
that turn it into a wrong kernel (test infrastructure).

tests/test_t5_tied_scores.py and tests/test_gpu_unigram_ties.py run the device tokenizer on
vocabularies whose scores tie (tests/golden/make_t5_tied_vocab.py).  A parity test on such
inputs is only worth something if a kernel that breaks a tie differently would fail it, so this
module restates the Viterbi in forty lines and offers the three ways a kernel is likely to get
it wrong; the tests count the words on which each wrong variant changes the ids.

The input is the bytes of "▁" + word, the pre-token after normalization: the model does not
normalize, so it is used only on words whose normalization is the identity, and every use
asserts first that the unswitched model equals the C oracle (oracle/orc_unigram.c).

The DP: starts ascending over char boundaries; per start the vocabulary's prefixes in
ascending length; cand = score + best[start]; a node is replaced when it is unset or
cand > best; the start's unk (min_score - 10) is tried, last, only when no one-char piece
starts there.  Then backtrack, fuse consecutive unks and look every string up (a fused run may
be a piece).  A duplicate piece string keeps its last id (a HashMap insert).

  strict=False       replaces on cand >= best: the last candidate wins a tie
  f32=True           piece scores rounded to f32: the one-ulp mark of a piece dropped
  reverse_sum=True   a path's score accumulated from its last piece to its first
"""
import struct

META = "▁".encode()


def _f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def u8len(b):
    return 1 if b < 0x80 else 2 if (b & 0xE0) == 0xC0 else 3 if (b & 0xF0) == 0xE0 else 4 if (b & 0xF8) == 0xF0 else 1


class PlainUnigram:
    def __init__(self, vocab, unk_id=2):
        """vocab: the tokenizer.json model's [piece, score] list (scores as `tokenizers` holds
        them: the caller passes what serde_json reads, see from_file)."""
        self.ids = {}
        for i, (p, _) in enumerate(vocab):
            self.ids[p.encode()] = i
        self.score = [float(s) for _, s in vocab]
        self.score32 = [_f32(s) for s in self.score]
        self.unk_id = unk_id
        self.unk_score = min(self.score) - 10.0
        self.maxlen = max(map(len, self.ids))

    @classmethod
    def from_file(cls, path):
        """From a tokenizer.json, its numbers read the way serde_json reads them."""
        import json

        import oracle_lib
        with open(path, encoding="utf-8") as f:
            model = json.load(f, parse_float=lambda t: oracle_lib.json_number(t))["model"]
        return cls(model["vocab"], model["unk_id"])

    def nodes(self, acc, strict=True, f32=False, reverse_sum=False):
        """The node table of acc: [(score, start, id)] per byte position, start -1 where unset."""
        n = len(acc)
        sc = self.score32 if f32 else self.score
        best = [(0.0, -1, -1)] * (n + 1)
        path = [()] * (n + 1)  # reverse_sum: the piece scores of the node's path

        def total(st, s):
            if not reverse_sum:
                return s + best[st][0]
            t = s
            for x in reversed(path[st]):
                t = t + x
            return t

        def relax(e, st, s, i):
            c = total(st, s)
            if best[e][1] < 0 or (c > best[e][0] if strict else c >= best[e][0]):
                best[e] = (c, st, i)
                if reverse_sum:
                    path[e] = path[st] + (s,)

        st = 0
        while st < n:
            mb = min(u8len(acc[st]), n - st)
            single = False
            for e in range(st + 1, min(st + self.maxlen, n) + 1):
                i = self.ids.get(acc[st:e])
                if i is None:
                    continue
                relax(e, st, sc[i], i)
                single = single or e - st == mb
            if not single:
                relax(st + mb, st, self.unk_score, self.unk_id)
            st += mb
        return best

    def encode(self, acc, **switches):
        """The ids of one pre-token (bytes of "▁" + word)."""
        best = self.nodes(acc, **switches)
        seq, e = [], len(acc)
        while e > 0:
            _, st, i = best[e]
            if i == self.unk_id and seq and seq[-1][2]:
                seq[-1][0] = st  # fuse the run leftwards
            else:
                seq.append([st, e, i == self.unk_id])
            e = st
        return [self.ids.get(acc[a:b], self.unk_id) for a, b, _ in reversed(seq)]

    def encode_word(self, word, **switches):
        return self.encode(META + (word.encode() if isinstance(word, str) else bytes(word)), **switches)
