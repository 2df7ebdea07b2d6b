#!/usr/bin/env python3
"""What prompt / completion examples (sdl_config.pair = 6, pack_prompt.hip) cost the packed clm rows,
on the same build: clm with pack = 1 at S=1024 B=128 and S=512 B=128 over the bench's 256 MiB arena,
its records taken two by two as (prompt, completion).  Per shape one handle with pair = 6 over the n
pairs and one plain packed handle over the same 2 n text ranges as records, both warmed up, their
steps alternated in one process and timed with device events on the stream the kernels run on; the
rows stage (everything after the tokenizer's stages: the lengths, the scan, the gather and the
carry) comes from sdl_stage_times in a pass of its own.

Per leg: the step and the rows stage (median and range of the runs), the rows and stream ids of one
call on an empty carry, the rows stage in ns a row; for the pair = 6 leg the share of the emitted
rows' label positions that are -100, and both times over the plain leg's.

    python tools/pack_prompt_bench.py [--arena-mib 256] [--runs 7] [--steps 5] [--out FILE.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench  # noqa: E402  (the arena builders of the headline benchmark)
import numpy as np  # noqa: E402
import pack_bench  # noqa: E402
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

SHAPES = ((1024, 128), (512, 128))
ROWS_STAGES = ("scan_rows", "rows")  # what follows `records`: the packed handles run it all under `rows`


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pack_prompt_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    R = len(order) // 2 * 2  # (an odd last record is left out of both legs)
    N = int(offs[R])
    text = torch.from_numpy(arena).to(dev)
    offsets = torch.from_numpy(offs[:R + 1].astype(np.int64)).to(dev)
    out = {"build_id": native.build_id(),
           "arena": {"arena_mib": args.arena_mib, "bytes": N, "text_ranges": R, "pairs": R // 2, "runs": args.runs,
                     "steps_per_run": args.steps},
           "shapes": {}}
    for S, BATCH in SHAPES:
        legs = {}
        for name, pair in (("plain", 0), ("prompt", native.SDL_PAIR_CLM_COMPLETION)):
            db = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=BATCH, sequence_length=S,
                               tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1, pair=pair)
            if pair:
                def step(db=db):
                    return db.process_pairs(text.data_ptr(), N, offsets.data_ptr(), R // 2, stream=stream.cuda_stream)
            else:
                def step(db=db):
                    return db.process(text.data_ptr(), N, offsets.data_ptr(), R, 0, stream.cuda_stream)
            legs[name] = (db, step)
        for db, step in legs.values():  # warm up every shape the timed window uses
            for _ in range(2):
                step()
                torch.cuda.synchronize(dev)
        step_ms = {name: [] for name in legs}
        for _ in range(args.runs):  # alternated: one run of each leg a round
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
        rows_ms = {name: [] for name in legs}
        for db, _ in legs.values():
            db.set_profiling(True)
        for _ in range(args.runs):
            for name, (db, step) in legs.items():
                step()
                torch.cuda.synchronize(dev)
                t = db.stage_times()
                rows_ms[name].append(sum(t.get(k, 0.0) for k in ROWS_STAGES))
        for db, _ in legs.values():
            db.set_profiling(False)
        shape = {"min_ids": int(legs["plain"][0].cfg.min_ids), "legs": {}}
        for name, (db, step) in legs.items():  # the counts, from one call on an empty carry
            db.flush_device(stream.cuda_stream)
            res = step()
            torch.cuda.synchronize(dev)
            rr = res.record_rows()
            rows = res.rows()
            med = statistics.median(rows_ms[name])
            lab = res.tensors(rows)["labels"]
            shape["legs"][name] = {
                "step_ms": pack_bench.med_range(step_ms[name]), "rows_stage_ms": pack_bench.med_range(rows_ms[name]),
                "rows": rows, "documents_kept": int((rr > 0).sum()), "tokenizer_ids": res.tokens(),
                "stream_ids": int(rr.sum()), "rows_stage_ns_per_row": round(med * 1e6 / rows, 3),
                "labels_minus_100_share": round(float((lab == -100).sum().item()) / lab.numel(), 6)}
        plain, prompt = shape["legs"]["plain"], shape["legs"]["prompt"]
        prompt["over_plain"] = {"step_time": round(prompt["step_ms"]["median"] / plain["step_ms"]["median"], 4),
                                "rows_stage_time": round(prompt["rows_stage_ms"]["median"] / plain["rows_stage_ms"]["median"], 4),
                                "rows_stage_ns_per_row": round(prompt["rows_stage_ns_per_row"] / plain["rows_stage_ns_per_row"], 4)}
        out["shapes"][f"S{S}_B{BATCH}"] = shape
        for db, _ in legs.values():
            db.close()
    text_out = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text_out + "\n")
    print(text_out)


if __name__ == "__main__":
    main()
