"""Object results on the device (efes_objects_results, DeviceObjects.verify) against sorting the per-extent sums and
statuses out on the host, in one GPU run: writes profiles/objects_results/bench.json and bench.log beside it.

    python tools/bench_objects_results.py [--out PATH] [--reps 15] [--seconds 0.3] [--shapes 0,1,2,3,4,5]

The shapes are the five of profiles/objects_jobs/bench.json by their counts: 32 768 x 4, 65 536 x 4, 4096 x 64, 65 536
objects of 1-8 extents and 262 144 x 4; and, for the failure path alone, ONE object of 1 048 576 extents.  The call
reads no data byte, so the sets are built from a device table (DeviceObjects.from_table) and not run: the sums are
random bytes and the expected digests the sums of the last extents.  The cases:
  none       -- every status EFES_OK, every digest as expected;
  differ     -- 1 % of the expected digests spoiled in one byte;
  failed     -- 1 % of the objects with one member, picked at random, whose status is EFES_ERR_ARG;
  all_failed -- EVERY member's status EFES_ERR_ARG: every lane of the per-extent pass searches its owner and takes the
                atomic minimum, 4 to 64 of them on one word, and all 1 048 576 on one word in the one-object shape.
Per shape and case, alternating in this process (repetition 0 is the warm-up):
  verify       -- DeviceObjects.verify(expected) with expected already on the device: the call, a synchronise, the 16
                  bytes of counts and then the bad list to the host; wall time.
  verify_up    -- the same with expected in host memory, so its upload (24 bytes per object) is included; wall time.
  host         -- the path the library offered before: sums.cpu() and status.cpu() (24 + 4 bytes per extent), then a
                  VECTORISED numpy pick (no Python loop): failures per object by add.reduceat over the statuses, the
                  sums of the last extents by one fancy index, one compare against expected; wall time.
  call         -- efes_objects_results alone (counts and bad list, no records), between two events; device time.
  call_records -- the same with the 32-byte records too; device time.
Before any figure is reported the bad list and the counters of the device path equal those of the host path and the
planted ones."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = [("32768 objects x 4 extents", lambda rng: np.full(32768, 4)),
          ("65536 objects x 4 extents", lambda rng: np.full(65536, 4)),
          ("4096 objects x 64 extents", lambda rng: np.full(4096, 64)),
          ("ragged: 65536 objects x 1-8 extents", lambda rng: rng.integers(1, 9, 65536)),
          ("262144 objects x 4 extents", lambda rng: np.full(262144, 4)),
          ("1 object x 1048576 extents (failure path only)", lambda rng: np.full(1, 1 << 20))]
CASES = ["none", "differ", "failed", "all_failed"]
ERR_ARG = -4


def spread(t: list[float]) -> dict:
    d = sorted(t[1:])
    return {"reps": len(d), "seconds_median": round(d[len(d) // 2], 7), "seconds_min": round(d[0], 7), "seconds_max": round(d[-1], 7)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_results", "bench.json"))
    ap.add_argument("--reps", type=int, default=15, help="timed repetitions of the wall-clock paths")
    ap.add_argument("--seconds", type=float, default=0.3, help="device-timed work of each call variant")
    ap.add_argument("--shapes", default="0,1,2,3,4,5")
    args = ap.parse_args()
    chosen = {int(x) for x in args.shapes.split(",")}

    import torch

    from efes_amd import _lib
    from efes_amd.batch import DeviceObjects
    from efes_amd.hashing import default_context, objects_results_scratch

    ctx = default_context(0)
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to("cuda:0")
    anchor = torch.zeros(256, dtype=torch.uint8, device="cuda:0")  # the table's data pointer: never dereferenced here
    results = []
    for si, (name, make) in enumerate(SHAPES):
        if si not in chosen:
            continue
        rng = np.random.default_rng(0xEFE5 + si)
        counts = np.asarray(make(rng), dtype=np.int64)
        m, n = len(counts), int(counts.sum())
        first = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
        starts, last = first[:-1].astype(np.int64), first[1:].astype(np.int64) - 1
        sums_h = rng.integers(0, 256, (n, 24), dtype=np.uint8)
        with torch.cuda.stream(stream):
            O = DeviceObjects.from_table(anchor.data_ptr(), torch.zeros((n, 2), dtype=torch.int64, device="cuda:0"),
                                         up(first).view(torch.int32), sha1=True, walk="wide", ctx=ctx)
            O.sums.copy_(up(sums_h).reshape(-1))
            O.status.zero_()
            scratch = torch.empty(objects_results_scratch(m, n), dtype=torch.uint8, device="cuda:0")
            bad_d = torch.empty(m, dtype=torch.int32, device="cuda:0")
            counts_d = torch.zeros(4, dtype=torch.int32, device="cuda:0")
            rec_d = torch.empty(32 * m, dtype=torch.uint8, device="cuda:0")
        stream.synchronize()
        row = {"shape": name, "objects": m, "extents": n, "host_path_bytes_to_host": 28 * n, "cases": []}
        for kind in CASES:
            if m == 1 and kind in ("differ", "failed"):
                continue  # 1 % of one object
            k = int(round(0.01 * m))
            status_h = np.zeros(n, np.int32)
            exp_h = sums_h[last].copy()
            if kind == "differ":
                planted = np.sort(rng.choice(m, k, replace=False))
                exp_h[planted, rng.integers(0, 24, k)] ^= 0x20
            elif kind == "failed":
                planted = np.sort(rng.choice(m, k, replace=False))
                status_h[starts[planted] + rng.integers(0, counts[planted])] = ERR_ARG
            elif kind == "all_failed":
                planted = np.arange(m)
                status_h[:] = ERR_ARG
            else:
                planted = np.zeros(0, np.int64)
            nfailed = len(planted) if kind in ("failed", "all_failed") else 0
            want_counts = [m - len(planted), len(planted) - nfailed, nfailed, 0]
            with torch.cuda.stream(stream):
                O.status[:n].copy_(up(status_h).view(torch.int32))
            exp_d = up(exp_h).reshape(m, 24)
            stream.synchronize()

            def host():
                sums = O.sums.cpu().numpy()[: 24 * n].reshape(n, 24)
                status = O.status.cpu().numpy()[:n]
                failed = np.add.reduceat((status != 0).astype(np.int32), starts) != 0  # every object has extents here
                differs = (sums[last] != exp_h).any(axis=1)
                return np.nonzero(failed | differs)[0], int(failed.sum())

            def call(records: bool):
                t = _lib.Objects(first=O._table_first.data_ptr(), sums=O.sums.data_ptr(), status=O.status.data_ptr(), nobjects=m, nextents=n)
                r = _lib.Results(expected=exp_d.data_ptr(), compare=3, results=rec_d.data_ptr() if records else None,
                                 bad=bad_d.data_ptr(), counts=counts_d.data_ptr())
                ctx.objects_results(t, r, scratch.data_ptr(), scratch.numel(), s)

            wall = {"verify": [], "verify_up": [], "host": []}
            with torch.cuda.stream(stream):
                for rep in range(args.reps + 1):
                    for p in wall:
                        stream.synchronize()
                        t0 = time.perf_counter()
                        if p == "host":
                            h_bad, h_failed = host()
                        else:
                            d_counts, d_bad = O.verify(exp_d if p == "verify" else exp_h)
                        wall[p].append(time.perf_counter() - t0)
                        if p != "host":
                            assert d_bad.tolist() == planted.tolist(), (name, kind, p, "bad list")
                            assert d_counts.tolist() == want_counts, (name, kind, p, d_counts)
                assert h_bad.tolist() == planted.tolist() and h_failed == nfailed, (name, kind, "host path")
                dev = {"call": [], "call_records": []}
                for rep in range(20000):
                    todo = [p for p in dev if rep < 2 or sum(dev[p][1:]) < args.seconds]
                    if not todo:
                        break
                    for p in todo:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        stream.synchronize()
                        e0.record(stream)
                        call(p == "call_records")
                        e1.record(stream)
                        stream.synchronize()
                        dev[p].append(e0.elapsed_time(e1) / 1e3)
                assert counts_d.cpu().tolist() == want_counts
                assert bad_d[: len(planted)].cpu().numpy().tolist() == planted.tolist()
            case = {"case": kind, "bad_objects": len(planted), "failed_members": int((status_h != 0).sum()), "verify_bytes_to_host": 16 + 4 * len(planted),
                    "wall": {p: spread(t) for p, t in wall.items()}, "device": {p: spread(t) for p, t in dev.items()}}
            for p in ("verify", "verify_up"):
                case[p + "_median_over_host_min"] = round(case["wall"][p]["seconds_median"] / case["wall"]["host"]["seconds_min"], 4)
            case["host_median_over_verify_min"] = round(case["wall"]["host"]["seconds_median"] / case["wall"]["verify"]["seconds_min"], 2)
            row["cases"].append(case)
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
        del O, scratch, bad_d, counts_d, rec_d, exp_d
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_objects_results.py", "device": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().efes_build_id().decode(), "wall_reps": args.reps, "seconds_per_device_path": args.seconds,
           "checks": ("the bad list and the counters of DeviceObjects.verify and of efes_objects_results equal the planted ones, and so does "
                      "the host path's list"),
           "shapes": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
