#!/usr/bin/env python3
"""What packed span rows (sdl_config.pack = 1 under the span task, pack_span.hip) cost against the
unpacked policy-1 rows of the same build (k_rows_span_t5, which this feature leaves as it was): span
at the bench shape (S=512, B=256), 150 per mille / mean 3.0, over the bench's fixture arena, both
handles warmed up, packed and unpacked steps alternated in one process and timed with device events
on the stream the kernels run on.  The tokenizer is shared, so the difference between the two steps
is the stage after it: per mode the step time (median and range of the runs), that stage and the
rows stage from the handle's own stage events (a second, profiled pass), rows written, the share
of filled input columns, the rows stage's ns per written row and ns per source id.

A row's source ids n come from its planes alone: filled input columns (u + m) plus label entries
(t + m + 1) is n + 2 m(n) + 1, which rises with n, so a table inverts it.

    python tools/pack_span_bench.py [--arena-mib 256] [--runs 5] [--steps 5] [--out FILE.json]

Prints one JSON document (and writes it to --out).  SDL_LIB=var/pack_span_abl{1,2}/libsdl_batcher.so
(build.py build_pack_span_ablations) times the diagnostic builds the same way."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench  # noqa: E402  (the arena builders and the step of the headline benchmark)
import pack_bench  # noqa: E402  (med_range)
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

S, BATCH = bench.TASKS["span"]["S"], bench.TASKS["span"]["B"]
PER_MILLE, MEAN = 150, 3.0
TOKENIZER_STAGES = ("chunk_ranges", "tokenize")


def counts(n):
    """span_noise_counts: (t, m) of a row of n ids."""
    if n < 2:
        return 0, 0
    t = min(max((n * PER_MILLE + 500) // 1000, 1), n - 1)
    return t, min(max(1, math.floor(t / MEAN + 0.5)), t, n - t)


def row_counts(torch, res, rows, top):
    """(filled input columns, source ids) of the first `rows` rows, counted on the device."""
    if rows == 0:
        return 0, 0
    t = res.tensors(rows)
    filled = (t["attention_mask"] == 1).sum(dim=1)
    entries = (t["labels"] != -100).sum(dim=1)
    inv = torch.zeros(top + 2 * counts(top)[1] + 2, dtype=torch.int64)
    for n in range(1, top + 1):
        inv[n + 2 * counts(n)[1] + 1] = n
    n = inv.to(filled.device)[filled + entries]
    assert int((n == 0).sum().item()) == 0
    return int(filled.sum().item()), int(n.sum().item())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pack_span_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    legs = {}
    for name, pack in (("unpacked", 0), ("packed", 1)):
        db = DeviceBatcher(task=native.SDL_TASK_SPAN, batch_size=BATCH, sequence_length=S, seed=1234,
                           tokenizer=native.T5_PROXY_TOKENIZER, avg_span_size=MEAN, span_policy=1,
                           span_noise_per_mille=PER_MILLE, pack=pack)
        legs[name] = (db, bench.make_step("span", db, records, arena, offs, order, first, dev, stream))
    N = int(native.load().sdl_pack_span_length(ctypes.byref(legs["packed"][0].cfg)))
    for db, step in legs.values():  # warm up every shape the timed window uses
        for _ in range(2):
            step()
            torch.cuda.synchronize(dev)
    step_ms = {name: [] for name in legs}
    for _ in range(args.runs):  # alternated: one run of each mode a round
        for name, (db, step) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record(stream)
            for _ in range(args.steps):
                step()
            e1.record(stream)
            e1.synchronize()
            step_ms[name].append(e0.elapsed_time(e1) / args.steps)
    # the stages, from the handle's events: a pass of its own, alternated like the steps
    stage_ms = {name: [] for name in legs}
    for db, _ in legs.values():
        db.set_profiling(True)
    for _ in range(args.runs):
        for name, (db, step) in legs.items():
            step()
            torch.cuda.synchronize(dev)
            stage_ms[name].append(db.stage_times())
    for db, _ in legs.values():
        db.set_profiling(False)
    out = {"build_id": native.build_id(), "lib": os.environ.get("SDL_LIB", "(the package's)"),
           "shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "span_policy": 1, "per_mille": PER_MILLE,
                     "mean": MEAN, "chunk_length": N, "runs": args.runs, "steps_per_run": args.steps,
                     "arena_bytes": len(arena) - 16, "records": len(order),
                     "min_ids": int(legs["packed"][0].cfg.min_ids)},
           "modes": {}}
    # the counts, from one call of each on an empty carry: rows, filled input columns, source ids
    for name, (db, step) in legs.items():
        if name == "packed":
            db.flush_device(stream.cuda_stream)
        res = step()
        torch.cuda.synchronize(dev)
        rows, toks = res.rows(), res.tokens()
        filled, src = row_counts(torch, res, rows, N)
        kept = int((res.record_rows() > 0).sum())
        stages = {k: pack_bench.med_range([s[k] for s in stage_ms[name]]) for k in stage_ms[name][0]}
        after = [sum(v for k, v in s.items() if k not in TOKENIZER_STAGES) for s in stage_ms[name]]
        rows_ms = stages["rows"]["median"]
        out["modes"][name] = {
            "step_ms": pack_bench.med_range(step_ms[name]), "stage_ms": stages,
            "after_tokenizer_ms": pack_bench.med_range(after), "rows": rows, "input_columns": rows * S,
            "filled_input_columns": filled, "filled_share": round(filled / (rows * S), 6) if rows else 0.0,
            "source_ids": src, "tokenizer_ids": toks, "records_kept": kept,
            "after_tokenizer_ns_per_row": round(statistics.median(after) * 1e6 / rows, 2) if rows else None,
            "rows_stage_ns_per_row": round(rows_ms * 1e6 / rows, 2) if rows else None,
            "rows_stage_ns_per_source_id": round(rows_ms * 1e6 / src, 4) if src else None}
    u, p = out["modes"]["unpacked"], out["modes"]["packed"]
    out["packed_over_unpacked"] = {
        "step_time": round(p["step_ms"]["median"] / u["step_ms"]["median"], 4),
        "after_tokenizer_time": round(p["after_tokenizer_ms"]["median"] / u["after_tokenizer_ms"]["median"], 4),
        "rows": round(p["rows"] / u["rows"], 4),
        "rows_stage_ns_per_row": round(p["rows_stage_ns_per_row"] / u["rows_stage_ns_per_row"], 4),
        "rows_stage_ns_per_source_id": round(p["rows_stage_ns_per_source_id"] / u["rows_stage_ns_per_source_id"], 4)}
    for db, _ in legs.values():
        db.close()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
