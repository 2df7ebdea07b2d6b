#!/usr/bin/env python3
"""What packed mlm rows (sdl_config.pack = 1 under the MLM task, pack_mlm.hip) cost against the
unpacked policy-1 rows of the same build: mlm at the bench shape (S=512, B=256), mask_policy 1,
over the bench's fixture arena, both handles warmed up, packed and unpacked steps alternated in one
process and timed with device events on the stream the kernels run on.  The tokenizer is shared,
so the difference between the two steps is the stage after it: per mode the step time (median and
range of the runs), that stage from the handle's own stage events (a second, profiled pass: the
events serialize nothing but are kept out of the step timing), rows written, the pad share of the
planes as counts, and the stage's ns per written row.

The unpacked rows keep the reference's reversed-range attention_mask (tools/pack_bench.py): a row
of l < S filled positions has l zeros, a full row none; the packed rows have the plain orientation.

    python tools/pack_mlm_bench.py [--arena-mib 256] [--runs 5] [--steps 5] [--out FILE.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import json
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

S, BATCH = bench.TASKS["mlm"]["S"], bench.TASKS["mlm"]["B"]
TOKENIZER_STAGES = ("chunk_ranges", "tokenize")


def pad_positions(res, rows, reversed_range):
    """Pad positions of the first `rows` rows, counted on the device (pack_bench.pad_positions at this S)."""
    if rows == 0:
        return 0
    z = (res.tensors(rows)["attention_mask"] == 0).sum(dim=1)
    return int((S - z[z > 0]).sum().item()) if reversed_range else int(z.sum().item())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pack_mlm_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    legs = {}
    for name, pack in (("unpacked", 0), ("packed", 1)):
        db = DeviceBatcher(batch_size=BATCH, sequence_length=S, seed=1234, mask_policy=1, pack=pack)
        legs[name] = (db, bench.make_step("mlm", db, records, arena, offs, order, first, dev, stream))
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
    out = {"build_id": native.build_id(),
           "shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "mask_policy": 1, "runs": args.runs,
                     "steps_per_run": args.steps, "arena_bytes": len(arena) - 16, "records": len(order),
                     "min_ids": int(legs["packed"][0].cfg.min_ids)},
           "modes": {}}
    # the counts, from one call of each on an empty carry: rows, pad positions, ids
    for name, (db, step) in legs.items():
        if name == "packed":
            db.flush_device(stream.cuda_stream)
        res = step()
        torch.cuda.synchronize(dev)
        rows, toks = res.rows(), res.tokens()
        pad = pad_positions(res, rows, name == "unpacked")
        kept = int((res.record_rows() > 0).sum())
        if name == "packed":
            assert pad == 0, f"{pad} padded positions in the packed call's full rows"
            fl = db.flush_device(stream.cuda_stream)
            torch.cuda.synchronize(dev)
            frows = fl.rows()
            rows, pad = rows + frows, pad_positions(fl, frows, False)
        stages = {k: pack_bench.med_range([s[k] for s in stage_ms[name]]) for k in stage_ms[name][0]}
        after = [sum(v for k, v in s.items() if k not in TOKENIZER_STAGES) for s in stage_ms[name]]
        positions = rows * S
        out["modes"][name] = {
            "step_ms": pack_bench.med_range(step_ms[name]), "stage_ms": stages,
            "after_tokenizer_ms": pack_bench.med_range(after), "rows": rows, "positions": positions,
            "pad_positions": pad, "pad_share": round(pad / positions, 6) if positions else 0.0, "tokenizer_ids": toks,
            "records_kept": kept,
            "after_tokenizer_ns_per_row": round(statistics.median(after) * 1e6 / rows, 2) if rows else None,
            "rows_stage_ns_per_row": round(stages["rows"]["median"] * 1e6 / rows, 2) if rows else None}
    u, p = out["modes"]["unpacked"], out["modes"]["packed"]
    out["packed_over_unpacked"] = {
        "step_time": round(p["step_ms"]["median"] / u["step_ms"]["median"], 4),
        "after_tokenizer_time": round(p["after_tokenizer_ms"]["median"] / u["after_tokenizer_ms"]["median"], 4),
        "rows": round(p["rows"] / u["rows"], 4),
        "after_tokenizer_ns_per_row": round(p["after_tokenizer_ns_per_row"] / u["after_tokenizer_ns_per_row"], 4)}
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
