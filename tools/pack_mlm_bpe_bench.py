#!/usr/bin/env python3
"""What the packed mlm rows over a byte-level BPE tokenizer in RoBERTa's form (pack_mlm_bpe.hip) cost
against the plain packed clm rows of the same build over the same records: B=128 at S=1024 (the clm
bench shape) or --seq 512, mask_policy 1 and 2, over the bench's fixture arena.  All three handles
are warmed up, their steps alternated in one process and timed with device events on the stream the
kernels run on.  The tokenizer kernels and their input are the same in every leg and both row
kernels move the same ids, so the difference between the `rows` stages is the policy's price: per
leg the step time (median and range of the runs), the stages from the handle's own events (a
second, profiled pass, kept out of the step timing), rows written, the rows stage's ns per written
row and the plane bytes it writes per second (4 planes a clm row, 5 an mlm row, 4 bytes each).

The RoBERTa-form tokenizer is derived from the gpt2 proxy in a temporary directory (roberta_form).

    python tools/pack_mlm_bpe_bench.py [--seq 1024] [--arena-mib 256] [--runs 5] [--steps 5] [--out FILE.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench  # noqa: E402  (the arena builders and the step of the headline benchmark)
import pack_bench  # noqa: E402  (med_range)
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

BATCH = bench.TASKS["clm"]["B"]
TOKENIZER_STAGES = ("chunk_ranges", "tokenize")
MASK_ID = 50260


def roberta_form(path):
    with open(native.GPT2_PROXY_TOKENIZER, encoding="utf-8") as f:
        j = json.load(f)
    eot = j["added_tokens"][0]
    eot["content"] = "</s>"
    j["added_tokens"] += [dict(eot, id=eot["id"] + 1 + k, content=c) for k, c in enumerate(("<s>", "<pad>", "<unk>", "<mask>"))]
    j["post_processor"] = {"type": "RobertaProcessing", "sep": ["</s>", eot["id"]], "cls": ["<s>", eot["id"] + 1],
                           "trim_offsets": True, "add_prefix_space": False}
    with open(path, "w", encoding="utf-8") as f:
        json.dump(j, f, ensure_ascii=False)
    return path


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--seq", type=int, default=bench.TASKS["clm"]["S"])
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pack_mlm_bpe_bench needs the GPU: nothing is measured without one")
    S = args.seq
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    tmp = tempfile.TemporaryDirectory()
    tok = roberta_form(os.path.join(tmp.name, "tokenizer.json"))
    legs = {}
    for name, kw in (("packed_clm", dict(task=native.SDL_TASK_CLM, tokenizer=native.GPT2_PROXY_TOKENIZER)),
                     ("packed_mlm_bpe_policy1", dict(tokenizer=tok, mask_policy=1, mask_id=MASK_ID)),
                     ("packed_mlm_bpe_policy2", dict(tokenizer=tok, mask_policy=2, mask_id=MASK_ID))):
        db = DeviceBatcher(batch_size=BATCH, sequence_length=S, seed=1234, pack=1, **kw)
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
    stage_ms = {name: [] for name in legs}
    for db, _ in legs.values():
        db.set_profiling(True)
    for _ in range(args.runs):
        for name, (db, step) in legs.items():
            step()
            torch.cuda.synchronize(dev)
            stage_ms[name].append(db.stage_times())
    out = {"build_id": native.build_id(),
           "shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "runs": args.runs, "steps_per_run": args.steps,
                     "arena_bytes": len(arena) - 16, "records": len(order), "min_ids": int(legs["packed_clm"][0].cfg.min_ids)},
           "legs": {}}
    for name, (db, step) in legs.items():  # the counts, from one unprofiled call on an empty carry
        db.set_profiling(False)
        db.flush_device(stream.cuda_stream)
        res = step()
        torch.cuda.synchronize(dev)
        rows, planes = res.rows(), 4 if name == "packed_clm" else 5
        stages = {k: pack_bench.med_range([s[k] for s in stage_ms[name]]) for k in stage_ms[name][0]}
        after = [sum(v for k, v in s.items() if k not in TOKENIZER_STAGES) for s in stage_ms[name]]
        rows_ms = stages["rows"]["median"]
        out["legs"][name] = {
            "step_ms": pack_bench.med_range(step_ms[name]), "stage_ms": stages,
            "after_tokenizer_ms": pack_bench.med_range(after), "rows": rows, "tokenizer_ids": res.tokens(),
            "records_kept": int((res.record_rows() > 0).sum()),
            "after_tokenizer_ns_per_row": round(statistics.median(after) * 1e6 / rows, 2),
            "rows_stage_ns_per_row": round(rows_ms * 1e6 / rows, 2),
            "rows_stage_plane_GBps": round(rows * S * planes * 4 / (rows_ms * 1e-3) / 1e9, 1)}
        db.close()
    clm = out["legs"]["packed_clm"]
    out["mlm_bpe_over_clm"] = {
        name: {"step_time": round(leg["step_ms"]["median"] / clm["step_ms"]["median"], 4),
               "rows_stage_time": round(leg["stage_ms"]["rows"]["median"] / clm["stage_ms"]["rows"]["median"], 4),
               "rows_stage_ns_per_row_added": round(leg["rows_stage_ns_per_row"] - clm["rows_stage_ns_per_row"], 2)}
        for name, leg in out["legs"].items() if name != "packed_clm"}
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
