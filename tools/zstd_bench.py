"""Measures sdl_zstd_inflate_device (the provider's zstd decode on the device).

    python tools/zstd_bench.py [--steps 10] [--warmup 3] [--mib 64] [--out FILE]

Two legs, each in a child process of its own under a time limit (a leg that faults or hangs ends the
run; nothing more is started on the GPU):

  many   a committed fixture frame of JSON lines (tests/golden/zstd/records_sum.zst) tiled to about
         --mib MiB of output -- a concatenation of frames is a valid .zst stream
  single one frame of about --mib MiB of JSON lines, made with libzstd (level 3) when one is found on
         the machine; otherwise reported as skipped

Times are HIP events around the call on the stream it runs on, medians over --steps after --warmup;
the per-stage split comes from sdl_set_profiling / sdl_stage_times in a further pass.  Beside them:
ZSTD_decompress of the same bytes on one CPU core, when a libzstd is found.  One JSON line per leg."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def leg(name, steps, warmup, mib):
    import numpy as np
    import torch
    import zstd_cases as zc
    from streaming_data_loader_amd import build, native
    from streaming_data_loader_amd.device import DeviceBatcher
    build.build()
    libs = zc.find_libzstd()
    lib = libs[0] if libs else None
    man = {e["name"]: e for e in zc.load_manifest()["fixtures"]}
    if name == "many":
        e = man["records_sum"]
        one, plain = zc.fixture_bytes(e), zc.fixture_plain(e)
        k = max(1, (mib << 20) // len(plain))
        z, want = one * k, plain * k
    else:
        if lib is None:
            return {"leg": name, "skipped": "no libzstd on this machine to make the frame"}
        src = zc.plaintext({"plain": "heldout"})
        want = (src * ((mib << 20) // len(src) + 1))[:mib << 20]
        want = want[:want.rfind(b"\n") + 1]
        z = lib.compress(want, level=3, checksum=True)
    off = native.zstd_split_frames(z)
    a = np.zeros(len(z) + 32, np.uint8)
    a[:len(z)] = np.frombuffer(z, np.uint8)
    dev = torch.device("cuda", 0)
    d_z = torch.from_numpy(a).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    db = DeviceBatcher(batch_size=8, sequence_length=128)
    stream = torch.cuda.current_stream(dev)
    n = len(off) - 1

    def call(flags=0):
        return db.zstd_inflate(d_z.data_ptr(), len(z), d_off.data_ptr(), n, flags=flags, stream=stream.cuda_stream)

    def timed(flags=0):
        for _ in range(warmup):
            out = call(flags)
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            out = call(flags)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return out, statistics.median(ms), min(ms)

    out, ms, ms_min = timed()
    assert int(out.out_bytes) == len(want) and int(out.n_bad) == 0
    got = np.zeros(len(want), np.uint8)
    native.d2h(db._h, got, out.d_out, got.nbytes)
    assert got.tobytes() == want, "device output differs from the plaintext"
    del got
    _, ms_nosum, _ = timed(native.SDL_ZSTD_NO_CHECKSUM)
    db.set_profiling(True)
    stages = {}
    for _ in range(max(3, steps // 2)):
        call()
        for k_, v in db.stage_times().items():
            stages.setdefault(k_, []).append(v)
    db.set_profiling(False)
    res = {"leg": name, "frames": n, "zst_bytes": len(z), "out_bytes": len(want), "ms": round(ms, 3),
           "ms_min": round(ms_min, 3), "out_GBps": round(len(want) / ms / 1e6, 3),
           "ms_no_checksum": round(ms_nosum, 3), "out_GBps_no_checksum": round(len(want) / ms_nosum / 1e6, 3),
           "stage_ms": {k_: round(statistics.median(v), 3) for k_, v in stages.items()},
           "steps": steps, "warmup": warmup, "build_id": native.build_id()}
    if lib is not None:
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            assert len(lib.decompress(z, len(want))) == len(want)
            t.append(time.perf_counter() - t0)
        res["libzstd"] = {"version": lib.version, "one_core_GBps": round(len(want) / min(t) / 1e9, 3)}
    else:
        res["libzstd"] = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--leg", choices=("many", "single"))
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.leg:
        print(json.dumps(leg(args.leg, args.steps, args.warmup, args.mib)), flush=True)
        return 0
    lines = []
    for name in ("many", "single"):
        cmd = ["timeout", "-k", "10", str(args.leg_timeout), sys.executable, os.path.abspath(__file__), "--leg", name,
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--mib", str(args.mib)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            print(json.dumps({"leg": name, "failed": p.returncode}), flush=True)
            return 1  # nothing more is started after a leg that failed
        line = p.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
