#!/usr/bin/env python3
"""What packed clm rows (sdl_config.pack = 1) cost and save against the unpacked rows, on the same
build: clm at the bench shape (S=1024, B=128) over the bench's 256 MiB arena, both handles warmed
up, packed and unpacked steps alternated in one process and timed with device events on the
stream the kernels run on.  Per mode: the step time (median and range of the runs), the pad share
as counts -- attention_mask == 0 positions over rows * S -- and non-pad ids per second.

The unpacked rows keep the reference's reversed-range attention_mask: a row that holds l < S ids
has its first l positions zeroed and the S - l padded ones set, so there the zero count of a row is
its filled length and the pad positions are S minus it (a full row has no zero).  Both counts are
reported for the unpacked rows; the packed rows have the plain orientation, where they coincide.

The packed pad share is at most one row's worth per call by construction (only the flush row is
padded); the tool asserts that count.

    python tools/pack_bench.py [--arena-mib 256] [--runs 5] [--steps 5] [--out FILE.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (the arena builders and the step of the headline benchmark)
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

S, BATCH = bench.TASKS["clm"]["S"], bench.TASKS["clm"]["B"]


def med_range(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def pad_positions(torch, res, rows, reversed_range):
    """(attention_mask == 0 positions, pad positions) of the first `rows` rows, counted on the device.
    reversed_range: the unpacked rows' attention_mask, whose zeros per row are the row's filled length."""
    if rows == 0:
        return 0, 0
    z = (res.tensors(rows)["attention_mask"] == 0).sum(dim=1)
    zeros = int(z.sum().item())
    return zeros, int((S - z[z > 0]).sum().item()) if reversed_range else zeros


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pack_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    legs = {}
    for name, pack in (("unpacked", 0), ("packed", 1)):
        db = DeviceBatcher(task=native.SDL_TASK_CLM, batch_size=BATCH, sequence_length=S, seed=1234,
                           tokenizer=native.GPT2_PROXY_TOKENIZER, pack=pack)
        legs[name] = (db, bench.make_step("clm", db, records, arena, offs, order, first, dev, stream))
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
    # the counts, from one call of each on an empty carry: rows, pad positions, ids
    out = {"shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "runs": args.runs, "steps_per_run": args.steps,
                     "arena_bytes": len(arena) - 16, "records": len(order), "min_ids": int(legs["packed"][0].cfg.min_ids)},
           "modes": {}}
    for name, (db, step) in legs.items():
        if name == "packed":
            db.flush_device(stream.cuda_stream)
        res = step()
        torch.cuda.synchronize(dev)
        rows, toks = res.rows(), res.tokens()
        zeros, pad = pad_positions(torch, res, rows, name == "unpacked")
        kept = int((res.record_rows() > 0).sum())
        if name == "packed":
            fl = db.flush_device(stream.cuda_stream)
            torch.cuda.synchronize(dev)
            frows = fl.rows()
            fpad = pad_positions(torch, fl, frows, False)[1]
            assert pad == 0, f"{pad} padded positions in the packed call's full rows"
            assert frows <= 1 and fpad < S, f"flush: {frows} rows, {fpad} padded positions"
            rows, pad, zeros = rows + frows, pad + fpad, zeros + fpad
        med = statistics.median(step_ms[name])
        positions = rows * S
        out["modes"][name] = {
            "step_ms": med_range(step_ms[name]), "rows": rows, "positions": positions, "attention_mask_zero_positions": zeros,
            "pad_positions": pad,
            "pad_share": round(pad / positions, 6) if positions else 0.0, "tokenizer_ids": toks,
            "records_kept": kept, "non_pad_ids": positions - pad,
            "non_pad_ids_per_s": round((positions - pad) / (med * 1e-3), 1),
            "text_GBps": round((len(arena) - 16) / (med * 1e-3) / 1e9, 2)}
    u, p = out["modes"]["unpacked"], out["modes"]["packed"]
    out["packed_over_unpacked"] = {"step_time": round(p["step_ms"]["median"] / u["step_ms"]["median"], 4),
                                   "rows": round(p["rows"] / u["rows"], 4),
                                   "non_pad_ids_per_s": round(p["non_pad_ids_per_s"] / u["non_pad_ids_per_s"], 4)}
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
