"""What the order of the chains in the job array costs the walks, and what making the longest-first order on the device
(efes_objects_order + efes_objects_jobs_ordered) costs and gains, in one GPU run: writes
profiles/objects_order/bench.json and bench.log beside it.

    python tools/bench_objects_order.py [--out PATH] [--reps 9] [--seconds 0.3] [--shapes 0,1,2,3]

The shapes are the ragged sets of profiles/hash_chain*/bench.json, each SHUFFLED by a fixed seed (those files sort them
longest first with numpy before building them), and one equal shape where an order can gain nothing, over a 4 GiB
synthetic pool.  Every set is fused (SHA-1 + CRC-32), FINALIZE on each object's last extent, and is walked by the call
DeviceObjects(walk="auto_wide") picks for its chain count: efes_hash_chain_wide from 32 chains per SIMD, else
efes_hash_chain_mode at efes_hash_chain_auto_mode's mode.  Per shape, alternating in this process (repetition 0 is the
warm-up); the table lies in device memory before any clock starts:
  leg 1  table    -- efes_objects_jobs on the shuffled table, then the walk: what the parent commit does with such a
                     table.  Device time of the walk alone ("walk_table") and of both ("table").
  leg 2  ordered  -- efes_objects_order + efes_objects_jobs_ordered + the walk, device time between two events
                     ("ordered"), and each call alone ("order_call", "ordered_build_call", "walk_ordered").
  leg 3  today    -- what a caller does today for the same order: first[] and the extents copied to the host, the sizes
                     by one cumulative sum, a numpy stable argsort, the table permuted on the host, uploaded,
                     efes_objects_jobs, the walk, a synchronise; WALL-CLOCK.  For the same clock, legs 1 and 2 are also
                     taken wall-clock, submit to synchronise ("wall").
  leg 4  presorted -- the walk over a table sorted on the host before it was built: the figure the header quoted so far
                     ("walk_presorted"), device time.
Before any figure is reported: the device order equals np.argsort(~sizes, kind="stable"); every status of every walk is
EFES_OK; the sums leg 2 leaves equal leg 1's byte for byte (both in table order); leg 4's, permuted back, equal them too.
"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_crc_batch import Probe  # noqa: E402
from bench_hash_chain import POOL, equal_shape, ragged_shape  # noqa: E402

SHUFFLE_SEED = 0x0DE2
SHAPES = [("ragged, shuffled: 65536 objects x 1-8 extents x 4 KiB-64 KiB", lambda: ragged_shape(0x4A66EF, 65536, 8, 64 << 10)),
          ("ragged, shuffled: 4096 objects x 1-16 extents x 4 KiB-256 KiB", lambda: ragged_shape(0x4A66EE, 4096, 16, 256 << 10)),
          ("ragged, shuffled: 1024 objects x 1-64 extents x 4 KiB-1 MiB", ragged_shape),
          ("equal, shuffled: 65536 objects x 4 extents x 16 KiB", lambda: equal_shape(65536, 4, 16 << 10))]


def spread(t: list[float]) -> dict:
    d = sorted(t[1:])
    return {"reps": len(d), "seconds_median": round(d[len(d) // 2], 7), "seconds_min": round(d[0], 7), "seconds_max": round(d[-1], 7)}


def packed(objects):
    counts = np.array([len(o) for o in objects], dtype=np.int64)
    ext = np.array([e for o in objects for e in o], dtype=np.uint64).reshape(int(counts.sum()), 2)
    return ext, np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)


def permuted(ext, first, order):
    """The table with its objects in `order`: what a host caller sorts and uploads today."""
    f = first.astype(np.int64)
    cnt = (f[1:] - f[:-1])[order]
    J = np.concatenate(([0], np.cumsum(cnt)))
    jmap = np.repeat(f[order] - J[:-1], cnt) + np.arange(int(J[-1]), dtype=np.int64)
    return ext[jmap], J.astype(np.uint32), jmap


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_order", "bench.json"))
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of the wall-clock paths")
    ap.add_argument("--seconds", type=float, default=0.3, help="device-timed work of every device path")
    ap.add_argument("--shapes", default="0,1,2,3")
    args = ap.parse_args()
    chosen = {int(x) for x in args.shapes.split(",")}

    import torch

    from efes_amd import _lib
    from efes_amd.hashing import (default_context, hash_chain_auto_mode_wide, hash_chain_scratch, objects_jobs_ordered_scratch,
                                  objects_jobs_scratch, objects_order_scratch)

    ctx = default_context(0)
    probe = Probe()
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    pool = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).to("cuda:0")
    results = []
    for si, (name, make) in enumerate(SHAPES):
        if si not in chosen:
            continue
        objects = make()
        np.random.default_rng(SHUFFLE_SEED + si).shuffle(objects)
        ext, first = packed(objects)
        del objects
        m, n = len(first) - 1, len(ext)
        E = np.concatenate((np.zeros(1, np.uint64), np.cumsum(ext[:, 1], dtype=np.uint64)))
        sizes = E[first[1:].astype(np.int64)] - E[first[:-1].astype(np.int64)]
        want_order = np.argsort(~sizes, kind="stable").astype(np.uint32)
        mode = hash_chain_auto_mode_wide(m, ctx)
        wide = mode == _lib.MODE_WIDE
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(pool.data_ptr(), POOL, 0x0DE2 + si, s)
            states = torch.zeros(m * 104, dtype=torch.uint8, device="cuda:0")
            crcs = torch.zeros(m * 4, dtype=torch.uint8, device="cuda:0")
            sums = torch.zeros(n * 24, dtype=torch.uint8, device="cuda:0")
            status = torch.full((n,), -99, dtype=torch.int32, device="cuda:0")
            jobs = torch.empty(n * 56, dtype=torch.uint8, device="cuda:0")
            order_d = torch.empty(m, dtype=torch.int32, device="cuda:0")
            scratch = torch.empty(max(hash_chain_scratch(n), objects_jobs_scratch(m, n), objects_jobs_ordered_scratch(m, n),
                                      objects_order_scratch(m, n)), dtype=torch.uint8, device="cuda:0")
            ext_d, first_d = up(ext), up(first)
            sext, sfirst, jmap = permuted(ext, first, want_order.astype(np.int64))  # leg 4's table
            sext_d, sfirst_d = up(sext), up(sfirst)
        stream.synchronize()
        sp, sb = scratch.data_ptr(), scratch.numel()

        def table_of(e_d, f_d):
            return _lib.Objects(data=pool.data_ptr(), extents=e_d.data_ptr(), first=f_d.data_ptr(), sha1=states.data_ptr(),
                                crc32=crcs.data_ptr(), sums=sums.data_ptr(), status=status.data_ptr(), nobjects=m, nextents=n,
                                flags=_lib.EFES_OBJECTS_FRESH)

        out = _lib.ObjectsOut(jobs=jobs.data_ptr())
        T, TS = table_of(ext_d, first_d), table_of(sext_d, sfirst_d)
        build = lambda t=T: ctx.objects_jobs(t, out, sp, sb, s)
        order_call = lambda: ctx.objects_order(T, order_d.data_ptr(), sp, sb, s)
        ordered_build = lambda: ctx.objects_jobs_ordered(T, out, order_d.data_ptr(), None, sp, sb, s)
        walk = (lambda: ctx.hash_chain_wide(jobs.data_ptr(), n, None, sp, sb, s)) if wide else \
               (lambda: ctx.hash_chain_mode(jobs.data_ptr(), n, sp, sb, s, mode))

        def leg1():
            build()
            walk()

        def leg2():
            order_call()
            ordered_build()
            walk()

        def today():  # from the table in device memory to the synchronise behind the walk
            f = first_d.cpu().numpy().view(np.uint32).astype(np.int64)
            e = ext_d.cpu().numpy().view(np.uint64).reshape(n, 2)
            acc = np.concatenate((np.zeros(1, np.uint64), np.cumsum(e[:, 1], dtype=np.uint64)))
            order = np.argsort(~(acc[f[1:]] - acc[f[:-1]]), kind="stable")
            pe, pf, _ = permuted(e, f.astype(np.uint32), order)
            pe_d, pf_d = up(pe), up(pf)
            build(table_of(pe_d, pf_d))
            walk()
            stream.synchronize()
            return pe_d, pf_d

        with torch.cuda.stream(stream):
            # ---- what the legs compute
            status.fill_(-99)
            leg1()
            stream.synchronize()
            assert bool((status == 0).all()), (name, "status, table order")
            sums_table = sums.clone()
            sums.zero_()
            status.fill_(-99)
            leg2()
            stream.synchronize()
            got_order = order_d.cpu().numpy().view(np.uint32)
            assert (got_order == want_order).all(), (name, "the device order is not numpy's")
            assert bool((status == 0).all()) and torch.equal(sums, sums_table), (name, "ordered sums differ from table-order sums")
            sums.zero_()
            build(TS)
            walk()
            stream.synchronize()
            back = torch.from_numpy(jmap).to("cuda:0")
            assert torch.equal(sums.view(n, 24), sums_table.view(n, 24)[back]), (name, "presorted sums")
            # ---- wall clock: legs 1, 2 and 3, submit to synchronise
            wall = {"table": [], "ordered": [], "today": []}
            for rep in range(args.reps + 1):
                for p, f in (("table", leg1), ("ordered", leg2), ("today", today)):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    keep = f()
                    stream.synchronize()
                    wall[p].append(time.perf_counter() - t0)
            del keep
            # ---- device time; a walk is timed over the job array its own build left
            dev = {k: [] for k in ("table", "walk_table", "ordered", "order_call", "ordered_build_call", "walk_ordered", "walk_presorted")}
            clock = {}
            prep = {"walk_table": build, "walk_ordered": lambda: (order_call(), ordered_build()), "walk_presorted": lambda: build(TS),
                    "ordered_build_call": order_call}
            runs = {"table": leg1, "walk_table": walk, "ordered": leg2, "order_call": order_call, "ordered_build_call": ordered_build,
                    "walk_ordered": walk, "walk_presorted": walk}
            for rep in range(20000):
                todo = [p for p in runs if rep < 2 or sum(dev[p][1:]) < args.seconds]
                if not todo:
                    break
                for p in todo:
                    if p in prep:
                        prep[p]()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    marked = probe.mark(s, 0)
                    e0.record(stream)
                    runs[p]()
                    e1.record(stream)
                    marked = marked and probe.mark(s, 1)
                    stream.synchronize()
                    dev[p].append(e0.elapsed_time(e1) / 1e3)
                    if marked:
                        clock[p] = probe.read()
            assert bool((status == 0).all()), (name, "status after the timed runs")
        stream.synchronize()
        row = {"shape": name, "objects": m, "extents": n, "hashed_bytes": int(ext[:, 1].sum()),
               "walk": "efes_hash_chain_wide" if wide else f"efes_hash_chain_mode({mode})",
               "wall": {p: spread(t) for p, t in wall.items()},
               "device": {p: {**spread(t), "engine_mhz": clock.get(p)} for p, t in dev.items()}}
        med = lambda k, p: row[k][p]["seconds_median"]
        low = lambda k, p: row[k][p]["seconds_min"]
        row["ordered_over_table"] = round(med("device", "ordered") / med("device", "table"), 4)
        row["ordered_median_below_table_min"] = med("device", "ordered") < low("device", "table")
        row["table_median_below_ordered_min"] = med("device", "table") < low("device", "ordered")
        row["walk_ordered_over_walk_table"] = round(med("device", "walk_ordered") / med("device", "walk_table"), 4)
        row["walk_ordered_over_walk_presorted"] = round(med("device", "walk_ordered") / med("device", "walk_presorted"), 4)
        row["ordered_over_walk_presorted"] = round(med("device", "ordered") / med("device", "walk_presorted"), 4)
        row["order_calls_over_walk_ordered"] = round((med("device", "order_call") + med("device", "ordered_build_call")) / med("device", "walk_ordered"), 4)
        row["ordered_wall_over_today_wall"] = round(med("wall", "ordered") / med("wall", "today"), 4)
        row["ordered_wall_median_below_today_wall_min"] = med("wall", "ordered") < low("wall", "today")
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
        del states, crcs, sums, sums_table, status, jobs, scratch, ext_d, first_d, sext_d, sfirst_d, order_d, back
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_objects_order.py", "device": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().efes_build_id().decode(),
           "engine_mhz": "per path, of its last repetition (tools/clockprobe.hip)", "pool_bytes": POOL,
           "wall_reps": args.reps, "seconds_per_device_path": args.seconds, "shuffle_seed": SHUFFLE_SEED,
           "checks": ("the device order equals np.argsort(~sizes, kind='stable'); every status of every walk is EFES_OK; the sums "
                      "of the ordered leg equal the table-order leg's byte for byte; the presorted leg's, permuted back, too"),
           "shapes": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
