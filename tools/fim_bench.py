#!/usr/bin/env python3
"""What fill-in-the-middle documents (sdl_batcher_set_fim) cost the packed clm rows, on the same
build: clm with pack = 1 at the bench shape (S=1024, B=128) over the bench's 256 MiB arena, one
handle without set_fim and one each for (rate, spm) per mille = (500, 500) and (1000, 0), all
warmed up, their steps alternated in one process and timed with device events on the stream the
kernels run on; the rows stage (everything after the tokenizer's stages: the lengths or the plan,
the scan, the gather and the carry) comes from sdl_stage_times in a pass of its own.

Per leg: the step and the rows stage (median and range of the runs), the rows and stream ids of one
call on an empty carry, the ids added against the plain leg, the rows stage in ns per stream id and
as bytes per second over the four planes it writes (16 bytes a stream id).

    python tools/fim_bench.py [--arena-mib 256] [--runs 7] [--steps 5] [--out FILE.json]

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
import pack_bench  # noqa: E402
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

S, BATCH = bench.TASKS["clm"]["S"], bench.TASKS["clm"]["B"]
LEGS = (("plain", None), ("fim_500_500", (500, 500)), ("fim_1000_0", (1000, 0)))
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
        sys.exit("fim_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    info = native.tokenizer_info(native.GPT2_PROXY_TOKENIZER)
    sent = [i for i in range(info.vocab_size - 1, -1, -1) if i != info.eos_id][:3]
    legs = {}
    for name, setting in LEGS:
        fim = None if setting is None else native.Fim(setting[0], setting[1], *sent)
        db = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=BATCH, sequence_length=S, seed=1234,
                           tokenizer=native.GPT2_PROXY_TOKENIZER, pack=1, fim=fim)
        legs[name] = (db, bench.make_step("clm", db, records, arena, offs, order, first, dev, stream))
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
    out = {"build_id": native.build_id(),
           "shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "runs": args.runs, "steps_per_run": args.steps,
                     "arena_bytes": len(arena) - 16, "records": len(order), "min_ids": int(legs["plain"][0].cfg.min_ids),
                     "sentinel_ids": sent},
           "legs": {}}
    for name, (db, step) in legs.items():  # the counts, from one call on an empty carry
        db.flush_device(stream.cuda_stream)
        res = step()
        torch.cuda.synchronize(dev)
        rr = res.record_rows()
        stream_ids = int(rr.sum())
        med = statistics.median(rows_ms[name])
        out["legs"][name] = {
            "step_ms": pack_bench.med_range(step_ms[name]), "rows_stage_ms": pack_bench.med_range(rows_ms[name]),
            "rows": res.rows(), "records_kept": int((rr > 0).sum()), "tokenizer_ids": res.tokens(), "stream_ids": stream_ids,
            "rows_stage_ns_per_stream_id": round(med * 1e6 / stream_ids, 5),
            "rows_stage_plane_GBps": round(16.0 * stream_ids / (med * 1e-3) / 1e9, 1),
            "rows_stage_plane_frac_of_hbm_peak": round(16.0 * stream_ids / (med * 1e-3) / 1e9 / bench.HBM_PEAK_GBPS, 4)}
    plain = out["legs"]["plain"]
    for name, leg in out["legs"].items():
        leg["ids_added"] = leg["stream_ids"] - plain["stream_ids"]
        leg["ids_added_share"] = round(leg["ids_added"] / plain["stream_ids"], 6)
        leg["over_plain"] = {"step_time": round(leg["step_ms"]["median"] / plain["step_ms"]["median"], 4),
                             "rows_stage_time": round(leg["rows_stage_ms"]["median"] / plain["rows_stage_ms"]["median"], 4)}
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
