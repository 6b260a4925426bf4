"""Chained CRC jobs against what a caller had before, in one GPU run: writes profiles/crc_chain/bench.json
and bench.log beside it.

    python tools/bench_crc_chain.py [--out PATH] [--seconds 1.0] [--shapes 0,1,2]

4 GiB of synthetic bytes per shape (well past the 256 MiB Infinity Cache), the paths alternating in
this process, each warmed once and then repeated until its device-event-timed work reaches --seconds.
  shape 1, 1024 x 4 MiB, no job flagged: efes_crc32_chain against efes_crc32_batch on the same job
      array (the tile kernel is shared: the finish launches differ).  The ratio is reported beside the
      batch path's own min-max spread over its repetitions.
  shapes 2 and 3, objects of 64 extents (64 x 64 x 1 MiB, 1024 x 64 x 64 KiB), three ways:
      (a) chain -- one efes_crc32_chain call, one state per object;
      (b) batch+fold -- efes_crc32_batch over the extents into piece states, the piece CRCs copied to the
          host and folded per object with efes_crc32_combine;
      (c) span -- one efes_crc32_span per extent into its object's state, all on one stream.
      Each is timed on the device (the launches alone) and on the host clock from the first launch to
      the last object's CRC in host memory; (a) and (c) copy their object CRCs to the host for that.
Before any rate is printed the object CRCs of all paths must be equal and two objects per shape must
match zlib.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POOL = 4 << 30
SHAPES = [("1024 x 4 MiB, unflagged", 1024, 1, 4 << 20), ("64 objects x 64 extents x 1 MiB", 64, 64, 1 << 20),
          ("1024 objects x 64 extents x 64 KiB", 1024, 64, 64 << 10)]


def stats(total: int, dev: list[float], wall: list[float]) -> dict:
    """Repetition 0 is the warm-up."""
    d, w = sorted(dev[1:]), sorted(wall[1:])
    return {"reps": len(d), "device_seconds_median": round(d[len(d) // 2], 6), "device_seconds_min": round(d[0], 6),
            "device_seconds_max": round(d[-1], 6), "device_GB_per_s": round(total / d[len(d) // 2] / 1e9, 1),
            "wall_seconds_median": round(w[len(w) // 2], 6), "wall_seconds_min": round(w[0], 6)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc_chain", "bench.json"))
    ap.add_argument("--seconds", type=float, default=1.0, help="device-timed work per path and shape")
    ap.add_argument("--shapes", default="0,1,2", help="which of the three shapes to run (a kernel trace wants one)")
    args = ap.parse_args()
    chosen = {int(x) for x in args.shapes.split(",")}

    import torch

    from efes_amd import _lib
    from efes_amd.hashing import crc32_batch_scratch, crc32_chain_scratch, crc32_combine, default_context

    ctx = default_context(0)
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    buf = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    results = []
    for si, (name, nobj, next_, size) in enumerate(SHAPES):
        if si not in chosen:
            continue
        n = nobj * next_
        assert n * size == POOL
        idx = np.arange(n, dtype=np.uint64)
        owner = idx // np.uint64(next_)
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(buf.data_ptr(), POOL, 0xC4A1 + si, s)
            obj = {p: torch.zeros(nobj, dtype=torch.int32, device="cuda:0") for p in ("chain", "span", "batch")}
            pieces = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            status = {p: torch.full((n,), -99, dtype=torch.int32, device="cuda:0") for p in ("chain", "batch")}
            host = {p: torch.zeros(nobj, dtype=torch.int32).pin_memory() for p in ("chain", "span", "batch")}
            host_pieces = torch.zeros(n, dtype=torch.int32).pin_memory()

            def job_array(states, per_job, flags, st):
                j = np.zeros(n, dtype=_lib.JOB_DTYPE)
                j["data"] = np.uint64(buf.data_ptr()) + idx * np.uint64(size)
                j["length"] = size
                j["crc32"] = np.uint64(states.data_ptr()) + (idx if per_job else owner) * np.uint64(4)
                j["status"] = np.uint64(st.data_ptr()) + idx * np.uint64(4)
                j["flags"] = flags
                return torch.from_numpy(j.view(np.uint8).copy()).to("cuda:0")

            heads = idx % np.uint64(next_) == 0  # every repetition starts from NewCRC32IEEE()
            chain_jobs = job_array(obj["chain"], False, np.where(heads, _lib.EFES_JOB_INIT, _lib.EFES_JOB_CHAIN).astype(np.uint32), status["chain"])
            batch_jobs = job_array(pieces if next_ > 1 else obj["batch"], True, _lib.EFES_JOB_INIT, status["batch"])
            chain_scratch = torch.empty(crc32_chain_scratch(n), dtype=torch.uint8, device="cuda:0")
            batch_scratch = torch.empty(crc32_batch_scratch(n), dtype=torch.uint8, device="cuda:0")
        stream.synchronize()
        fold_seconds = []

        def run_chain():
            ctx.crc32_chain(chain_jobs.data_ptr(), n, chain_scratch.data_ptr(), chain_scratch.numel(), s)
            return lambda: host["chain"].copy_(obj["chain"], non_blocking=True)

        def run_batch():
            ctx.crc32_batch(batch_jobs.data_ptr(), n, batch_scratch.data_ptr(), batch_scratch.numel(), s)
            if next_ == 1:
                return lambda: host["batch"].copy_(obj["batch"], non_blocking=True)
            return lambda: host_pieces.copy_(pieces, non_blocking=True)

        def fold():  # the piece CRCs are on the host: crc32.go's Writes, merged
            t0 = time.perf_counter()
            out = host["batch"].numpy().view(np.uint32)
            for i, p in enumerate(host_pieces.numpy().view(np.uint32).reshape(nobj, next_).tolist()):
                crc = p[0]
                for piece in p[1:]:
                    crc = crc32_combine(crc, piece, size)
                out[i] = crc
            fold_seconds.append(time.perf_counter() - t0)

        def run_span():
            obj["span"].zero_()
            for k in range(n):
                ctx.crc32_span(buf.data_ptr() + k * size, size, obj["span"].data_ptr() + 4 * (k // next_), s)
            return lambda: host["span"].copy_(obj["span"], non_blocking=True)

        paths = {"chain": run_chain, "batch": run_batch}
        if next_ > 1:
            paths["span"] = run_span
        dev = {p: [] for p in paths}
        wall = {p: [] for p in paths}
        with torch.cuda.stream(stream):
            for rep in range(20000):
                todo = [p for p in paths if rep < 2 or sum(dev[p][1:]) < args.seconds]
                if not todo:
                    break
                for p in todo:  # alternating; repetition 0 is the warm-up
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    t0 = time.perf_counter()
                    e0.record(stream)
                    copy_back = paths[p]()
                    e1.record(stream)
                    copy_back()
                    stream.synchronize()
                    if p == "batch" and next_ > 1:
                        fold()
                    wall[p].append(time.perf_counter() - t0)
                    dev[p].append(e0.elapsed_time(e1) / 1e3)
        stream.synchronize()
        # ---- correctness before any rate
        got = {p: host[p].numpy().view(np.uint32).copy() for p in paths}
        for p in paths:
            assert (got[p] == got["chain"]).all(), (name, p, np.nonzero(got[p] != got["chain"])[0][:5])
            if p in status:
                assert (status[p].cpu().numpy() == 0).all(), (name, p)
        for i in {0, nobj - 1}:
            a, m = i * next_ * size, next_ * size
            assert zlib.crc32(buf[a:a + m].cpu().numpy()) == int(got["chain"][i]), (name, i)
        row = {"shape": name, "objects": nobj, "extents_per_object": next_, "jobs": n, "bytes": POOL,
               "paths": {p: stats(POOL, dev[p], wall[p]) for p in paths}}
        a, b = row["paths"]["chain"], row["paths"]["batch"]
        if next_ == 1:
            row["chain_over_batch_device"] = round(a["device_seconds_median"] / b["device_seconds_median"], 4)
            row["batch_spread_min_max_over_median"] = [round(b["device_seconds_min"] / b["device_seconds_median"], 4),
                                                       round(b["device_seconds_max"] / b["device_seconds_median"], 4)]
        else:
            f = sorted(fold_seconds[1:])
            b["host_fold_seconds_median"] = round(f[len(f) // 2], 6)
            c = row["paths"]["span"]
            row["batch_fold_wall_over_chain_wall"] = round(b["wall_seconds_median"] / a["wall_seconds_median"], 2)
            row["span_wall_over_chain_wall"] = round(c["wall_seconds_median"] / a["wall_seconds_median"], 2)
            row["span_device_over_chain_device"] = round(c["device_seconds_median"] / a["device_seconds_median"], 2)
            row["chain_device_over_batch_device"] = round(a["device_seconds_median"] / b["device_seconds_median"], 4)
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
    out = {"tool": "tools/bench_crc_chain.py", "device": torch.cuda.get_device_name(0), "build_id": _lib.lib().efes_build_id().decode(),
           "pool_bytes": POOL, "seconds_per_path": args.seconds,
           "checks": "all paths' object CRCs equal; two objects per shape equal zlib", "shapes": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
