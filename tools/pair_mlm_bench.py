#!/usr/bin/env python3
"""What MLM sentence pairs (sdl_config.pair 2..4) cost, at the mlm shape of a BERT pre-training
batch: S=128, B=2048, mask_policy 1, over the bench's arena.  Four legs over the same device arena
and offsets: its records taken two by two as pairs under pair = 2 (as given), 3 (next-sentence
draws) and 4 (sentence-order draws), and the same 2 n records unpaired through mask_policy 1 on a
pair = 0 handle.  The tokenizer's work is identical in all four.  Before anything is timed, every
pair handle's planes and pair labels of a sample call (the arena's first pairs) are compared with
tests/pair_mlm_model.py, exactly.  Handles warmed up, the legs alternated in one process, timed
with device events on the stream the kernels run on.

Per leg: the step time and the stage after the tokenizer (sdl_stage_times of profiled steps run
beside the timed ones: every stage from scan_chunks on), median and range over the runs, the rows,
and the four planes' bytes over the stage time.

The yardstick is the unpaired leg on the build of the commit before the feature: run this tool
there (or with SDL_LIB naming that build's library) with --unpaired-only --out PARENT.json, then
here with --parent-json PARENT.json; the parent's leg is filed as "unpaired_parent" and the
ratios are taken against it.

    python tools/pair_mlm_bench.py [--arena-mib 256] [--runs 5] [--steps 5] [--unpaired-only]
                                   [--parent-json FILE] [--out FILE.json]

Prints one JSON document (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import bench  # noqa: E402  (the arena builder of the headline benchmark)
from streaming_data_loader_amd import native  # noqa: E402
from streaming_data_loader_amd.device import DeviceBatcher  # noqa: E402

S, BATCH, POLICY, PER_MILLE, SEED = 128, 2048, 1, 150, 1234
MASK_LENGTH = int(np.float32(S) * np.float32(0.15))
SAMPLE_PAIRS = 96
PAIR_LEGS = {"pair_2_as_given": 2, "pair_3_nsp": 3, "pair_4_sop": 4}


def med_range(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def after_tokenizer(stages):
    names = list(stages)
    return sum(stages[n] for n in names[names.index("tokenize") + 1:])


def verify_sample(torch, dev, db, mode, arena, offs, first):
    """The first SAMPLE_PAIRS pairs as a call of their own against the model (exact)."""
    import oracle_lib
    import pair_mlm_model as M
    tok = oracle_lib.Tok()
    n = SAMPLE_PAIRS
    N = int(offs[2 * n])
    texts = [bytes(arena[int(offs[q]):int(offs[q + 1])]) for q in range(2 * n)]
    ids = [tok.encode(t)[1:-1] for t in texts]
    pairs = [(ids[2 * r], ids[2 * r + 1]) for r in range(n)]
    want = M.rows(pairs, S, mode, POLICY, SEED, first, MASK_LENGTH, PER_MILLE, B=BATCH)
    text = torch.from_numpy(arena[:N + 16].copy()).to(dev)
    offsets = torch.from_numpy(offs[:2 * n + 1].astype(np.int64)).to(dev)
    res = db.process_pairs(text.data_ptr(), N, offsets.data_ptr(), n, first_record=first)
    torch.cuda.synchronize(dev)
    G = want["planes"].shape[1]
    if res.rows() != n:
        sys.exit(f"pair = {mode}: {res.rows()} rows of {n} pairs")
    for name, g, w in zip(("input_ids", "attention_mask", "token_type_ids", "labels"), res.planes(G), want["planes"]):
        if not np.array_equal(g, w):
            sys.exit(f"pair = {mode}: {name} differs from the model on the sample call")
    if not np.array_equal(res.pair_labels(G), want["pair_labels"]):
        sys.exit(f"pair = {mode}: the pair labels differ from the model on the sample call")
    return {"pairs": n, "picked": int((want["planes"][3][:n] != -100).sum()), "label_1": int(want["pair_labels"][:n].sum())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arena-mib", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--unpaired-only", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("pair_mlm_bench needs the GPU: nothing is measured without one")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    records, arena, offs, order, first = bench.shard(0, args.arena_mib << 20, "fixture", 1)
    R = len(order) - len(order) % 2  # an even number of records: every leg sees the same text
    n_pairs, N = R // 2, int(offs[R])
    text = torch.from_numpy(arena).to(dev)
    offsets = torch.from_numpy(offs[:R + 1].astype(np.int64)).to(dev)

    def make(pair):
        return DeviceBatcher(task=native.SDL_TASK_MLM, batch_size=BATCH, sequence_length=S, seed=SEED,
                             mask_policy=POLICY, mask_per_mille=PER_MILLE, mask_length=MASK_LENGTH, pair=pair)

    legs, verified = {}, {}
    db = make(0)
    legs["unpaired"] = (db, lambda db=db: db.process(text.data_ptr(), N, offsets.data_ptr(), R, first, stream.cuda_stream))
    if not args.unpaired_only:
        for name, mode in PAIR_LEGS.items():
            db = make(mode)
            verified[name] = verify_sample(torch, dev, db, mode, arena, offs, first)
            legs[name] = (db, lambda db=db: db.process_pairs(text.data_ptr(), N, offsets.data_ptr(), n_pairs,
                                                             first_record=first, stream=stream.cuda_stream))
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
    out = {"shape": {"arena_mib": args.arena_mib, "S": S, "B": BATCH, "mask_policy": POLICY, "mask_per_mille": PER_MILLE,
                     "mask_length": MASK_LENGTH, "runs": args.runs, "steps_per_run": args.steps, "text_bytes": N,
                     "records": R, "pairs": n_pairs},
           "build_id": native.build_id(), "hbm_peak_GBps": bench.HBM_PEAK_GBPS, "sample_verified": verified, "legs": {}}
    for name, (db, step) in legs.items():
        res = step()
        torch.cuda.synchronize(dev)
        rows = res.rows()
        padded = -(-rows // BATCH) * BATCH
        plane_bytes = 4 * padded * S * 4  # four int32 planes written once
        med, tail = statistics.median(step_ms[name]), statistics.median(tail_ms[name])
        leg = {"step_ms": med_range(step_ms[name]), "after_tokenizer_ms": med_range(tail_ms[name]),
               "stages_ms": {k: round(statistics.median(s[k] for s in stages[name]), 4) for k in stages[name][0]},
               "rows": rows, "rows_written": padded, "tokenizer_ids": res.tokens(), "plane_bytes": plane_bytes,
               "planes_over_after_tokenizer_GBps": round(plane_bytes / (tail * 1e-3) / 1e9, 1),
               "after_tokenizer_ns_per_row": round(tail * 1e6 / max(padded, 1), 2),
               "text_GBps": round(N / (med * 1e-3) / 1e9, 2)}
        if name != "unpaired":
            lab = res.pair_labels(rows)
            leg["label_1_share"] = round(float((lab == 1).mean()), 4) if rows else 0.0
        out["legs"][name] = leg
        db.close()
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        out["legs"]["unpaired_parent"] = dict(parent["legs"]["unpaired"], build_id=parent.get("build_id"))
    yard = out["legs"].get("unpaired_parent", out["legs"]["unpaired"])
    out["yardstick"] = "unpaired_parent" if args.parent_json else "unpaired"
    out["over_yardstick"] = {
        name: {"step_time": round(leg["step_ms"]["median"] / yard["step_ms"]["median"], 4),
               "after_tokenizer": round(leg["after_tokenizer_ms"]["median"] / yard["after_tokenizer_ms"]["median"], 4),
               "after_tokenizer_per_row": round(leg["after_tokenizer_ns_per_row"] / yard["after_tokenizer_ns_per_row"], 4)}
        for name, leg in out["legs"].items() if leg is not yard}
    text_out = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text_out + "\n")
    print(text_out)


if __name__ == "__main__":
    main()
