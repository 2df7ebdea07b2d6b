#!/usr/bin/env python3
"""What T5's span corruption (sdl_config.span_policy 1, 150 per mille, mean span 3.0) costs beside
the reference's rule (policy 0, Span{16.0, 2.0}) on the same build: the `rows` stage
(sdl_stage_times) and the whole step at the span bench shape (256 MiB arena, S=512, B=256),
medians and ranges of alternated runs, their ratios, and what each policy makes of a row -- the
share of non-pad input positions and of labels that are not -100 over the filled rows.

    python tools/span_policy_bench.py [--arena-mib 256] [--runs 5] [--steps 5] [--out FILE.json]

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
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

S, BATCH = 512, 256
POLICIES = {0: dict(avg_span_gap=16.0, avg_span_size=2.0, span_policy=0, span_noise_per_mille=0),
            1: dict(avg_span_gap=16.0, avg_span_size=3.0, span_policy=1, span_noise_per_mille=150)}


def med_range(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--corpus", default="fixture")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, args.corpus, 1)
    legs = {}
    for p, kw in POLICIES.items():
        db = DeviceBatcher(task=native.SDL_TASK_SPAN, batch_size=BATCH, sequence_length=S, seed=1234,
                           tokenizer=native.T5_PROXY_TOKENIZER, **kw)
        legs[p] = (db, bench.make_step("span", db, records, arena, offs, order, first, dev, stream))
    for db, step in legs.values():
        for _ in range(2):
            res = step()
            torch.cuda.synchronize(dev)
    step_ms = {p: [] for p in legs}
    rows_ms = {p: [] for p in legs}
    stages = {}
    made = {}
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
            st = db.stage_times()
            rows_ms[p].append(st.get("rows", float("nan")))
            stages[p] = {k: round(v, 4) for k, v in st.items()}
            db.set_profiling(False)
            if p not in made:  # what the policy makes of the rows (the planes of this step, on the device)
                n = res.rows()
                t = res.tensors(n)
                made[p] = {"rows": n, "label_errors": res.label_errors(), "tokenize_errors": res.tokenize_errors(),
                           "input_nonpad_share": round(float((t["input_ids"] != 0).sum().item()) / (n * S), 4),
                           "attention_share": round(float(t["attention_mask"].sum().item()) / (n * S), 4),
                           "labels_used_share": round(float((t["labels"] != -100).sum().item()) / (n * (S // 4)), 4)}
                del t
    doc = {"shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "runs": args.runs, "steps_per_run": args.steps},
           "corpus": args.corpus, "arena_bytes": len(arena) - 16, "records": len(order),
           "config": {str(p): kw for p, kw in POLICIES.items()}, "policies": {}}
    for p in legs:
        padded = -(-made[p]["rows"] // BATCH) * BATCH
        plane_bytes = padded * (2 * S + S // 4) * 4  # input_ids, attention_mask and the S/4 labels, written once
        rows_med = statistics.median(rows_ms[p])
        doc["policies"][str(p)] = dict(made[p], step_ms=med_range(step_ms[p]), rows_stage_ms=med_range(rows_ms[p]),
                                       rows_stage_write_GBps=round(plane_bytes / (rows_med * 1e-3) / 1e9, 1),
                                       stages_ms_last_profiled_step=stages[p])
    r0, r1 = doc["policies"]["0"], doc["policies"]["1"]
    doc["policy1_over_policy0"] = {
        "rows_stage": round(r1["rows_stage_ms"]["median"] / r0["rows_stage_ms"]["median"], 3),
        "step": round(r1["step_ms"]["median"] / r0["step_ms"]["median"], 3)}
    for db, _ in legs.values():
        db.close()
    text = json.dumps(doc, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
