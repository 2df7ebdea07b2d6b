#!/usr/bin/env python3
"""Times the WordPiece path under the uncased and the cased proxy tokenizer at one commit.

The arena is bench.py's (the corpus records tiled in seeded permutations, 256 MiB by default);
each run is --steps calls of sdl_process_device (mlm, S=512, B=256) with sdl_set_profiling
stage times, and the two tokenizers' runs alternate (uncased, cased, uncased, ...), --runs of
each after a warm-up.  The vocabularies differ, so their pending-word rates do: the words a
chunk that miss the first-piece table are estimated on the CPU from tokenizers' word groups
over the corpus records (a word that is one ASCII piece of <= 14 bytes, or one punctuation
char, is taken as not pending: an estimate, not the kernel's count) and reported next to the
times.

    python tools/wordpiece_settings_bench.py --corpus fixture --out profiles/r12/cased/fixture.json
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

TOKENIZERS = {"uncased": native.BERT_PROXY_TOKENIZER, "cased": native.BERT_CASED_PROXY_TOKENIZER}


def pending_per_chunk(path, records):
    from tokenizers import Tokenizer
    tok = Tokenizer.from_file(path)
    pending = nbytes = 0
    for t in records:
        enc = tok.encode(t, add_special_tokens=False)
        groups = {}
        for piece, w in zip(enc.tokens, enc.word_ids):
            groups.setdefault(w, []).append(piece)
        for g in groups.values():
            p = g[0]
            if len(g) == 1 and p.isascii() and p != "[UNK]" and (len(p) <= 14 if p.isalnum() else len(p) == 1):
                continue
            pending += 1
        nbytes += len(t.encode("utf-8"))
    return 1024.0 * pending / nbytes


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", default="fixture", choices=["fixture", "heldout"])
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, args.corpus, 1)
    N, R = len(arena) - 16, len(order)
    text = torch.from_numpy(arena).cuda()
    off = torch.from_numpy(offs.astype("int64")).cuda()
    dbs = {k: DeviceBatcher(batch_size=256, sequence_length=512, seed=1234, tokenizer=p) for k, p in TOKENIZERS.items()}

    def run(db, steps, timed):
        tok = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            res = db.process(text.data_ptr(), N, off.data_ptr(), R, first)
            if timed:
                tok += db.stage_times().get("tokenize", 0.0)
        torch.cuda.synchronize()
        assert res.tokenize_errors() == 0
        return {"step_ms": (time.perf_counter() - t0) / steps * 1e3, "tokenize_ms": tok / steps, "ids": res.tokens()}

    for db in dbs.values():
        run(db, args.warmup, False)
        db.set_profiling(True)
    runs = {k: [] for k in dbs}
    for _ in range(args.runs):
        for k, db in dbs.items():
            runs[k].append(run(db, args.steps, True))
    out = {"corpus": args.corpus, "arena_bytes": N, "records": R, "steps_per_run": args.steps,
           "build": native.build_id()[:16], "device": torch.cuda.get_device_name(0)}
    for k in dbs:
        out[k] = {"pending_words_per_chunk_cpu": round(pending_per_chunk(TOKENIZERS[k], records), 2),
                  "ids": runs[k][0]["ids"]}
        for m in ("step_ms", "tokenize_ms"):
            v = [r[m] for r in runs[k]]
            out[k][m] = {"runs": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                         "min": round(min(v), 4), "max": round(max(v), 4)}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
