#!/usr/bin/env python3
"""What best-fit rows (sdl_batcher_set_best_fit) cost and buy against the plain packed clm rows, on the
same build (pack.hip is the parent's, byte for byte): clm with pack = 1 at the bench shape over the
bench's 256 MiB arena, one handle without the call and one each for W = 256, 1024 and 4096, all
warmed up, their steps alternated in one process and timed with device events on the stream the
kernels run on; the rows stage (everything after the tokenizer's stages: lengths or plan, scan, rows)
comes from sdl_stage_times in a pass of its own.

Per leg: the step and the rows stage (median and range of the runs), the rows of one call, the pad
share (columns with attention 0 among the emitted rows) and the share of kept documents that do not
lie whole in one row -- from d_record_rows (where each document lies) and checked against the pieces
that position_ids and attention_mask show.

    python tools/best_fit_bench.py [--arena-mib 256] [--runs 7] [--steps 5] [--out FILE.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench  # noqa: E402  (the arena builders and the step of the headline benchmark)
import pack_bench  # noqa: E402
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

S, BATCH = bench.TASKS["clm"]["S"], bench.TASKS["clm"]["B"]
LEGS = (("plain", None), ("best_fit_256", 256), ("best_fit_1024", 1024), ("best_fit_4096", 4096))
ROWS_STAGES = ("scan_rows", "rows")  # what follows `records`: the packed handles run it all under `rows`


def layout(res, W):
    """(pad share, cut share, pieces) of one call's rows on an empty carry."""
    G = res.rows()
    _, am, _, _ = res.planes(G)
    pos = res.position_ids(G)
    L = res.record_rows().astype(np.int64)
    kept = L > 0
    if W is None:  # the stream: document r lies at [start, start + L)
        start = np.cumsum(L) - L
        first, last = start // S, (start + L - 1) // S
        cut = kept & (first != last)
        pieces = int((np.minimum(last, G - 1) - first + 1)[kept & (first < G)].sum())  # (what lies behind row G waits in the carry)
    else:
        cut = L > S
        pieces = int((-(-L // S))[kept].sum())
    seen = int(((pos == 0) & (am == 1)).sum())
    return round(float((am == 0).mean()), 6), round(float(cut.sum() / max(kept.sum(), 1)), 6), pieces, seen


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("best_fit_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    legs = {}
    for name, W in LEGS:
        db = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=BATCH, sequence_length=S, seed=1234,
                           tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1,
                           best_fit=None if W is None else native.BestFit(W))
        legs[name] = (db, bench.make_step("clm", db, records, arena, offs, order, first, dev, stream), W)
    for db, step, _ in legs.values():  # warm up every shape the timed window uses
        for _ in range(2):
            step()
            torch.cuda.synchronize(dev)
    step_ms = {name: [] for name in legs}
    for _ in range(args.runs):  # alternated: one run of each leg a round
        for name, (db, step, _) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            e0.record(stream)
            for _ in range(args.steps):
                step()
            e1.record(stream)
            e1.synchronize()
            step_ms[name].append(e0.elapsed_time(e1) / args.steps)
    # the stages, from the handle's events: a pass of its own, alternated like the steps
    rows_ms = {name: [] for name in legs}
    for db, _, _ in legs.values():
        db.set_profiling(True)
    for _ in range(args.runs):
        for name, (db, step, _) in legs.items():
            step()
            torch.cuda.synchronize(dev)
            t = db.stage_times()
            rows_ms[name].append(sum(t.get(k, 0.0) for k in ROWS_STAGES))
    for db, _, _ in legs.values():
        db.set_profiling(False)
    out = {"build_id": native.build_id(),
           "shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "runs": args.runs, "steps_per_run": args.steps,
                     "arena_bytes": len(arena) - 16, "records": len(order), "min_ids": int(legs["plain"][0].cfg.min_ids)},
           "legs": {}}
    for name, (db, step, W) in legs.items():  # the layout, from one call on an empty carry
        db.flush_device(stream.cuda_stream)
        res = step()
        torch.cuda.synchronize(dev)
        pad, cut, pieces, seen = layout(res, W)
        rr = res.record_rows()
        out["legs"][name] = {
            "window_records": W, "step_ms": pack_bench.med_range(step_ms[name]),
            "rows_stage_ms": pack_bench.med_range(rows_ms[name]), "rows": res.rows(),
            "records_kept": int((rr > 0).sum()), "segment_ids": int(rr.sum()), "pad_share": pad,
            "cut_documents_share": cut, "pieces_from_record_rows": pieces, "pieces_in_planes": seen}
    plain = out["legs"]["plain"]
    for leg in out["legs"].values():
        leg["over_plain"] = {"step_time": round(leg["step_ms"]["median"] / plain["step_ms"]["median"], 4),
                             "rows_stage_time": round(leg["rows_stage_ms"]["median"] / plain["rows_stage_ms"]["median"], 4),
                             "rows": round(leg["rows"] / plain["rows"], 4)}
    for db, _, _ in legs.values():
        db.close()
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
