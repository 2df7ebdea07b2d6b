#!/usr/bin/env python3
"""What the BERT masking policies (sdl_config.mask_policy 1 / 2) cost over the reference policy,
on the same build: the `rows` stage (sdl_stage_times) and the whole step at the mlm bench shape
(256 MiB arena, S=512, B=256), policies 0 / 1 / 2 on the fixture corpus and 0 / 2 on the held-out
corpus (only that text splits words into pieces, so only there the whole-word skip loop works),
medians and ranges of alternated runs; the rows stage against the HBM bound of its plane writes;
and the time of a per-record push under policy 1 against policy 0 (the policies' small calls take
a rows launch of their own).

    python tools/mlm_policy_bench.py [--arena-mib 256] [--runs 5] [--steps 5] [--out FILE.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (the arena builders and the step of the headline benchmark)
from streaming_data_loader_amd import batcher as B  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

S, BATCH = 512, 256


def med_range(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def device_leg(args, torch, dev, stream, corpus, policies):
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, corpus, 1)
    legs = {}
    for p in policies:
        db = DeviceBatcher(batch_size=BATCH, sequence_length=S, seed=1234, mask_policy=p, mask_per_mille=150)
        legs[p] = (db, bench.make_step("mlm", db, records, arena, offs, order, first, dev, stream))
    for db, step in legs.values():
        for _ in range(2):
            res = step()
            torch.cuda.synchronize(dev)
    step_ms = {p: [] for p in policies}
    rows_ms = {p: [] for p in policies}
    n_rows = {}
    for _ in range(args.runs):  # alternated: one run of every policy a round
        for p, (db, step) in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                res = step()
            torch.cuda.synchronize(dev)
            step_ms[p].append((time.perf_counter() - t0) / args.steps * 1e3)
            db.set_profiling(True)  # (a profiled step is not a timed one: the events serialise the stages)
            res = step()
            torch.cuda.synchronize(dev)
            rows_ms[p].append(db.stage_times().get("rows", float("nan")))
            db.set_profiling(False)
            n_rows[p] = res.rows()
    out = {"corpus": corpus, "arena_bytes": len(arena) - 16, "records": len(order), "policies": {}}
    for p in policies:
        padded = -(-n_rows[p] // BATCH) * BATCH
        plane_bytes = 4 * padded * S * 4  # four int32 planes written once
        rows_med = statistics.median(rows_ms[p])
        out["policies"][str(p)] = {
            "rows": n_rows[p], "step_ms": med_range(step_ms[p]), "rows_stage_ms": med_range(rows_ms[p]),
            "rows_stage_write_GBps": round(plane_bytes / (rows_med * 1e-3) / 1e9, 1),
            "rows_stage_frac_of_hbm_peak": round(plane_bytes / (rows_med * 1e-3) / 1e9 / bench.HBM_PEAK_GBPS, 3)}
    for db, _ in legs.values():
        db.close()
    return out


def push_leg(args, policies, n_records=2000):
    """Per-record create_sync_batch (host in, host out), microseconds a record."""
    records = bench.fixture_records()
    texts = [records[i % len(records)] for i in range(n_records)]
    us = {p: [] for p in policies}
    for _ in range(args.runs):
        for p in policies:
            gt = B.GenTokenizer(B.ModelType.Bert, B.BatchConfig(BATCH, S), B.Mask(76, 103, p, 150), B.TokenizerConfig(),
                                chunk=True, seed=1234)
            for t in texts[:200]:
                gt.create_sync_batch(t)
            t0 = time.perf_counter()
            for t in texts:
                gt.create_sync_batch(t)
            us[p].append((time.perf_counter() - t0) / len(texts) * 1e6)
            gt.close()
    return {str(p): med_range(us[p]) for p in policies}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    doc = {"shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "runs": args.runs, "steps_per_run": args.steps},
           "hbm_peak_GBps": bench.HBM_PEAK_GBPS,
           "fixture": device_leg(args, torch, dev, stream, "fixture", (0, 1, 2)),
           "heldout": device_leg(args, torch, dev, stream, "heldout", (0, 2)),
           "per_record_push_us": push_leg(args, (0, 1))}
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
