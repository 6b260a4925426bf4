"""The object-table builder (efes_objects_jobs) against building the chain calls' arrays on the host, in one GPU run:
writes profiles/objects_jobs/bench.json and bench.log beside it.

    python tools/bench_objects_jobs.py [--out PATH] [--reps 9] [--seconds 0.3] [--shapes 0,1,2,3,4]

The shapes are those of profiles/hash_chain_wide/bench.json, so that the numbers sit beside the walks they feed:
32 768 x 4 x 32 KiB, 65 536 x 4 x 16 KiB, 262 144 x 4 x 4 KiB, 4096 x 64 x 4 KiB and the ragged 65 536 objects of 1-8
extents of 4-64 KiB, over a 4 GiB synthetic pool.  Every set is fused (SHA-1 + CRC-32), FINALIZE on every extent,
with a record per extent and the default gather layout, so all three arrays -- jobs, dst[], ckpt[] -- are made.
Per shape, alternating in this process (repetition 0 is the warm-up):
  host    -- what DeviceObjects(build="host") does from PACKED numpy arrays (ext (n, 2), counts): the field-by-field
             fill of the JOB_DTYPE array, the record and destination pointers, three uploads, a synchronise; wall time.
             The gather layout is taken vectorised here (cumulative sums), which favours this path: the constructor
             loops over the objects in Python (default_copy_offsets).
  lists   -- the Python-list work in front of it in the constructor, reported separately: the flattening of the lists
             into ext and counts, and default_copy_offsets; wall time.
  ctor    -- for scale, the whole constructors from the Python lists, build="host" and build="device"; wall time.
  device  -- from the same packed arrays: first[] by one cumulative sum, the upload of the 16 + 4 byte table, the
             allocation of the three arrays, efes_objects_jobs, a synchronise; wall time.
  call    -- efes_objects_jobs alone, between two events; device time.  bytes = what it must read (16 per extent, 4
             per object) plus what it must write (72 per extent, 8 per object); its share of the 8 TB/s HBM peak.
  walk    -- efes_hash_chain_wide on the job array the builder made, without records; device time: the builder as a
             fraction of the walk it precedes.
Before any figure is reported the device-built arrays equal the host-built ones byte for byte (the same base
addresses go into both), the layout equals default_copy_offsets', and every status of the walk is EFES_OK.
"""
from __future__ import annotations

import argparse
import ctypes
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

HBM_PEAK = 8e12  # bytes per second (MI355X)
SHAPES = [("32768 objects x 4 extents x 32 KiB", lambda: equal_shape(32768, 4, 32 << 10)),
          ("65536 objects x 4 extents x 16 KiB", lambda: equal_shape(65536, 4, 16 << 10)),
          ("262144 objects x 4 extents x 4 KiB", lambda: equal_shape(262144, 4, 4 << 10)),
          ("4096 objects x 64 extents x 4 KiB", lambda: equal_pool(4096, 64, 4 << 10)),
          ("ragged: 65536 objects x 1-8 extents x 4 KiB-64 KiB, longest first", lambda: ragged_shape(0x4A66EF, 65536, 8, 64 << 10))]


def equal_pool(nobj: int, next_: int, size: int):
    """equal_shape for a set smaller than the pool: consecutive extents from the pool's start."""
    return [[((i * next_ + k) * size, size) for k in range(next_)] for i in range(nobj)]


def spread(t: list[float]) -> dict:
    d = sorted(t[1:])
    return {"reps": len(d), "seconds_median": round(d[len(d) // 2], 6), "seconds_min": round(d[0], 6), "seconds_max": round(d[-1], 6)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_jobs", "bench.json"))
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of the wall-clock paths")
    ap.add_argument("--seconds", type=float, default=0.3, help="device-timed work of the call and of the walk")
    ap.add_argument("--shapes", default="0,1,2,3,4")
    args = ap.parse_args()
    chosen = {int(x) for x in args.shapes.split(",")}

    import torch

    from efes_amd import _lib
    from efes_amd.batch import COPY_ALIGN, DeviceObjects, default_copy_offsets
    from efes_amd.hashing import default_context, hash_chain_scratch, objects_jobs_scratch

    FIN, INIT, CHAIN = _lib.EFES_JOB_FINALIZE, _lib.EFES_JOB_INIT, _lib.EFES_JOB_CHAIN
    REC = _lib.CHECKPOINT_DTYPE.itemsize
    ctx = default_context(0)
    probe = Probe()
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    pool = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    up = lambda a: torch.from_numpy(a.view(np.uint8)).to("cuda:0")
    results = []
    for si, (name, make) in enumerate(SHAPES):
        if si not in chosen:
            continue
        objects = make()
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(pool.data_ptr(), POOL, 0x0B1E + si, s)
            m = len(objects)
            n = sum(len(o) for o in objects)
            states = torch.zeros(m * 104, dtype=torch.uint8, device="cuda:0")
            crcs = torch.zeros(m * 4, dtype=torch.uint8, device="cuda:0")
            sums = torch.zeros(n * 24, dtype=torch.uint8, device="cuda:0")
            status = torch.full((n,), -99, dtype=torch.int32, device="cuda:0")
            recs = torch.zeros(n * REC, dtype=torch.uint8, device="cuda:0")
            scratch = torch.empty(max(hash_chain_scratch(n), objects_jobs_scratch(m, n)), dtype=torch.uint8, device="cuda:0")
            copy_to = 0x7000_0000_0000  # only added to: nothing here gathers
        stream.synchronize()

        def lists():  # the constructor's work on the Python lists
            objs = [list(o) for o in objects]
            counts = np.array([len(o) for o in objs], dtype=np.int64)
            ext = np.array([e for o in objs for e in o], dtype=np.uint64).reshape(int(counts.sum()), 2)
            offsets, room = default_copy_offsets(objs)
            return ext, counts, offsets, room

        ext, counts, want_offsets, want_room = lists()
        assert len(ext) == n and (want_offsets % COPY_ALIGN == 0).all()

        def host():  # DeviceObjects.__init__'s fill from the packed arrays, then the three uploads
            first = np.concatenate(([0], np.cumsum(counts)))[:-1]
            last = first + counts - 1
            owner = np.repeat(np.arange(m, dtype=np.uint64), counts)
            idx = np.arange(n, dtype=np.uint64)
            jobs = np.zeros(n, dtype=_lib.JOB_DTYPE)
            jobs["data"] = np.uint64(pool.data_ptr()) + ext[:, 0]
            jobs["length"] = ext[:, 1]
            jobs["crc32"] = np.uint64(crcs.data_ptr()) + owner * np.uint64(4)
            jobs["sha1"] = np.uint64(states.data_ptr()) + owner * np.uint64(104)
            jobs["sum"] = np.uint64(sums.data_ptr()) + idx * np.uint64(24)
            jobs["status"] = np.uint64(status.data_ptr()) + idx * np.uint64(4)
            jobs["flags"] = CHAIN
            jobs["flags"][first[counts > 0]] = INIT
            jobs["flags"] |= FIN
            at = np.uint64(recs.data_ptr()) + idx * np.uint64(REC)
            before = np.cumsum(ext[:, 1]) - ext[:, 1]
            own = owner.astype(np.int64)
            within = before - before[first[own]]
            sizes = np.add.reduceat(ext[:, 1], first) if n else np.zeros(m, np.uint64)  # every object has extents here
            rounded = (sizes + np.uint64(COPY_ALIGN - 1)) & ~np.uint64(COPY_ALIGN - 1)
            offsets = np.cumsum(rounded) - rounded
            dst = np.uint64(copy_to) + offsets[own] + within
            out = up(jobs), up(dst.astype(np.uint64)), up(at.astype(np.uint64))
            torch.cuda.synchronize()
            return out, offsets, last

        def table():
            first = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
            return up(ext), up(first)

        def call(ext_d, first_d, jobs, dst, ck, layout):
            t = _lib.Objects(data=pool.data_ptr(), extents=ext_d.data_ptr(), first=first_d.data_ptr(), sha1=states.data_ptr(),
                             crc32=crcs.data_ptr(), sums=sums.data_ptr(), status=status.data_ptr(), ckpt=recs.data_ptr(),
                             copy_to=copy_to, nobjects=m, nextents=n,
                             flags=_lib.EFES_OBJECTS_FRESH | _lib.EFES_OBJECTS_RUNNING, copy_align=COPY_ALIGN)
            o = _lib.ObjectsOut(jobs=jobs.data_ptr(), dst=dst.data_ptr(), ckpt=ck.data_ptr(), layout=layout.data_ptr())
            ctx.objects_jobs(t, o, scratch.data_ptr(), scratch.numel(), s)

        def outputs():
            return (torch.empty(n * 56, dtype=torch.uint8, device="cuda:0"), torch.empty(n * 8, dtype=torch.uint8, device="cuda:0"),
                    torch.empty(n * 8, dtype=torch.uint8, device="cuda:0"), torch.empty(m + 1, dtype=torch.int64, device="cuda:0"))

        def device():
            ext_d, first_d = table()
            out = outputs()
            call(ext_d, first_d, *out)
            torch.cuda.synchronize()
            return out

        wall = {"host": [], "device": [], "lists": [], "ctor_host": [], "ctor_device": []}
        with torch.cuda.stream(stream):
            for rep in range(args.reps + 1):
                for p, f in (("host", host), ("device", device)):
                    t0 = time.perf_counter()
                    keep = f()
                    wall[p].append(time.perf_counter() - t0)
                    if p == "host":
                        (hj, hd, hc), h_offsets, _ = keep
                    else:
                        dj, dd, dc, dl = keep
            for rep in range(3):
                t0 = time.perf_counter()
                lists()
                wall["lists"].append(time.perf_counter() - t0)
                for build in ("host", "device"):
                    t0 = time.perf_counter()
                    O = DeviceObjects(pool.data_ptr(), objects, running=True, sha1=True, ctx=ctx, walk="wide", checkpoints=True,
                                      copy_to=copy_to, build=build)
                    torch.cuda.synchronize()
                    wall["ctor_" + build].append(time.perf_counter() - t0)
                    del O
            # ---- the arrays of the two paths are the same bytes
            assert torch.equal(hj, dj) and torch.equal(hd, dd) and torch.equal(hc, dc), (name, "arrays differ")
            lay = dl.cpu().numpy().view(np.uint64)
            assert (lay[:-1] == want_offsets).all() and int(lay[-1]) == want_room and (h_offsets == want_offsets).all(), (name, "layout")
            # ---- device time of the call alone, and of the walk behind it
            ext_d, first_d = table()
            dev, clock = {"call": [], "walk": []}, {}
            runs = {"call": lambda: call(ext_d, first_d, dj, dd, dc, dl),
                    "walk": lambda: ctx.hash_chain_wide(dj.data_ptr(), n, None, scratch.data_ptr(), scratch.numel(), s)}
            for rep in range(20000):
                todo = [p for p in runs if rep < 2 or sum(dev[p][1:]) < args.seconds]
                if not todo:
                    break
                for p in todo:
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
            assert torch.equal(hj, dj), (name, "the timed calls changed the jobs")
            assert bool((status == 0).all()), (name, "status")
        stream.synchronize()
        moved = (16 + 72) * n + (4 + 8) * (m + 1)
        row = {"shape": name, "objects": m, "extents": n, "hashed_bytes": int(ext[:, 1].sum()),
               "host_build_uploaded_bytes": 72 * n, "table_uploaded_bytes": 16 * n + 4 * (m + 1), "call_bytes_read_plus_written": moved,
               "wall": {p: spread(t) if p in ("host", "device") else spread([t[0]] + t) for p, t in wall.items()},
               "device": {p: {**spread(t), "engine_mhz": clock.get(p)} for p, t in dev.items()}}
        med = lambda k, p: row[k][p]["seconds_median"]
        row["device_wall_over_host_wall"] = round(med("wall", "device") / med("wall", "host"), 4)
        row["device_wall_median_below_host_wall_min"] = med("wall", "device") < row["wall"]["host"]["seconds_min"]
        row["call_GB_per_s"] = round(moved / med("device", "call") / 1e9, 1)
        row["call_share_of_hbm_peak"] = round(moved / med("device", "call") / HBM_PEAK, 4)
        row["call_over_walk"] = round(med("device", "call") / med("device", "walk"), 4)
        row["host_wall_over_walk"] = round(med("wall", "host") / med("device", "walk"), 2)
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
        del states, crcs, sums, status, recs, scratch, hj, hd, hc, dj, dd, dc, dl, ext_d, first_d, keep
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_objects_jobs.py", "device": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().efes_build_id().decode(),
           "engine_mhz": "per path, of its last repetition (tools/clockprobe.hip)", "pool_bytes": POOL,
           "wall_reps": args.reps, "seconds_per_device_path": args.seconds, "hbm_peak_bytes_per_s": HBM_PEAK,
           "checks": ("the device-built jobs, dst[] and ckpt[] equal the host-built ones byte for byte; the layout equals "
                      "default_copy_offsets'; every status of efes_hash_chain_wide over the device-built jobs is EFES_OK"),
           "shapes": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
