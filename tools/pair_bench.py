#!/usr/bin/env python3
"""What sentence pairs (sdl_config.pair = 1) cost against the unpaired rows, on the same build:
single-class at the bench shape (S=128, B=2048) over the bench's arena.  Two legs over the same
device arena and offsets: its records taken two by two as pairs on a pair handle, and the same
2 n records unpaired on a pair = 0 handle.  The tokenizer's work is identical; the pair leg writes
half the rows.  Both handles warmed up, the legs alternated in one process and timed with device
events on the stream the kernels run on.

Per leg: the step time and the stage after the tokenizer (sdl_stage_times of profiled steps run
beside the timed ones: every stage from scan_chunks on), median and range over the runs, and the
pad share.  For the pair leg also the share of pairs that longest_first truncated, counted from a
call of the same pairs at S = 2048, where n_a + n_b shows in the attention mask.

    python tools/pair_bench.py [--arena-mib 256] [--runs 5] [--steps 5] [--out FILE.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402

import bench  # noqa: E402  (the arena builder of the headline benchmark)
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

S, BATCH = bench.TASKS["single-class"]["S"], bench.TASKS["single-class"]["B"]
S_WIDE = 2048  # the widest row a handle takes: n_a + n_b up to 2045 shows untruncated


def med_range(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def after_tokenizer(stages):
    names = list(stages)
    return sum(stages[n] for n in names[names.index("tokenize") + 1:])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pair_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    R = len(order) - len(order) % 2  # an even number of records: both legs see the same text
    n_pairs, N = R // 2, int(offs[R])
    text = torch.from_numpy(arena).to(dev)
    offsets = torch.from_numpy(offs[:R + 1].astype(np.int64)).to(dev)
    lab = torch.from_numpy((np.asarray(order[:R], np.int64) & 1).astype(np.int32)).to(dev)
    loff = torch.arange(R + 1, dtype=torch.int64, device=dev)

    def make(pair, seq=S):
        return DeviceBatcher(task=native.SDL_TASK_SINGLE_CLASS, batch_size=BATCH, sequence_length=seq, pair=pair)

    def pair_step(db):
        return lambda: db.process_pairs(text.data_ptr(), N, offsets.data_ptr(), n_pairs, lab.data_ptr(),
                                        loff.data_ptr(), first, stream.cuda_stream)

    def plain_step(db):
        return lambda: db.process_labels(text.data_ptr(), N, offsets.data_ptr(), R, lab.data_ptr(), loff.data_ptr(),
                                         first, stream.cuda_stream)

    legs = {}
    for name, mk in (("unpaired", plain_step), ("pairs", pair_step)):
        db = make(name == "pairs")
        legs[name] = (db, mk(db))
    for db, step in legs.values():  # warm up every shape the timed window uses, profiled and not
        for prof in (False, True, False):
            db.set_profiling(prof)
            step()
            torch.cuda.synchronize(dev)
    step_ms = {name: [] for name in legs}
    tail_ms = {name: [] for name in legs}
    stages = {name: [] for name in legs}
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
            db.set_profiling(True)  # (one profiled step a run, outside the timed window)
            step()
            torch.cuda.synchronize(dev)
            st = db.stage_times()
            db.set_profiling(False)
            stages[name].append(st)
            tail_ms[name].append(after_tokenizer(st))
    out = {"shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "runs": args.runs, "steps_per_run": args.steps,
                     "text_bytes": N, "records": R, "pairs": n_pairs}, "legs": {}}
    for name, (db, step) in legs.items():
        res = step()
        torch.cuda.synchronize(dev)
        rows = res.rows()
        z = (res.tensors(rows)["attention_mask"] == 0).sum(dim=1)
        # (the unpaired rows keep the reference's reversed range: a row's zeros are its filled length)
        pad = int(z.sum().item()) if name == "pairs" else int((S - z[z > 0]).sum().item())
        med = statistics.median(step_ms[name])
        out["legs"][name] = {
            "step_ms": med_range(step_ms[name]), "after_tokenizer_ms": med_range(tail_ms[name]),
            "stages_ms": {k: round(statistics.median(s[k] for s in stages[name]), 4) for k in stages[name][0]},
            "rows": rows, "tokenizer_ids": res.tokens(), "pad_positions": pad,
            "pad_share": round(pad / (rows * S), 6) if rows else 0.0,
            "text_GBps": round(N / (med * 1e-3) / 1e9, 2)}
    for db, _ in legs.values():
        db.close()
    wide = make(True, S_WIDE)
    res = pair_step(wide)()
    torch.cuda.synchronize(dev)
    ids_both = res.tensors(n_pairs)["attention_mask"].sum(dim=1) - 3  # n_a + n_b, up to S_WIDE - 3
    truncated = int((ids_both > S - 3).sum().item())
    wide.close()
    p, u = out["legs"]["pairs"], out["legs"]["unpaired"]
    p["pairs_truncated"] = truncated
    p["truncated_share"] = round(truncated / n_pairs, 6) if n_pairs else 0.0
    out["pairs_over_unpaired"] = {
        "step_time": round(p["step_ms"]["median"] / u["step_ms"]["median"], 4),
        "after_tokenizer": round(p["after_tokenizer_ms"]["median"] / u["after_tokenizer_ms"]["median"], 4),
        "step_ms_difference": round(p["step_ms"]["median"] - u["step_ms"]["median"], 4),
        "unpaired_step_range_ms": round(u["step_ms"]["max"] - u["step_ms"]["min"], 4)}
    text_out = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text_out + "\n")
    print(text_out)


if __name__ == "__main__":
    main()
