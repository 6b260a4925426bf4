"""PATCH logs on the device (efes_patches_table) against the host twin, in one GPU run: writes profiles/patches/bench.json
and bench.log beside it.

    python tools/bench_patches.py [--out PATH] [--reps 9] [--seconds 0.3] [--shapes 65536x4,262144x4,4096x64,1048576x1,1x1048576]

A shape is uploads x PATCHes per upload.  The logs are interleaved (a random arrival order that keeps every upload's own
order) and well-formed: half the uploads are new (their first PATCH comes at offset 0 and restarts them), half resume at a
stored offset, every PATCH continues its upload, half the uploads' last PATCH carries the length (DONE); bodies of 1 KiB
in a 256 MiB pool.  "conflicts" is the same with 1 % of the records replaced by PATCHes at an offset their upload never
reaches (409).  Per shape and log, alternating in this process (repetition 0 is the warm-up; every buffer exists
beforehand, so no path pays for an allocation):
    call    -- efes_patches_table alone, between two events; device time.
    builder -- efes_objects_jobs over the table the call made; device time.
    walk    -- efes_hash_chain_wide over the jobs (both digests); device time; not for the one-upload row, whose single
               chain of 2^20 extents no walk is meant for.
    device  -- the log (40 bytes per PATCH) and the offsets from host memory to the device, the call, a synchronise; wall.
    host    -- efes_patches_table_host, then extents, first and the reset states to the device, a synchronise; wall.
and what the zero-length slots cost: the walk over the table of a log with 10 % refused PATCHes against the walk over the
same table compacted on the host.  A path "wins" where its median is below the other's minimum.  Before any figure is
reported every output of the device call equals the host twin's byte for byte."""
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

BODY = 1024
POOL = 256 << 20
UNKNOWN = (1 << 64) - 1


def spread(t: list[float]) -> dict:
    d = sorted(t[1:])
    return {"reps": len(d), "seconds_median": round(d[len(d) // 2], 7), "seconds_min": round(d[0], 7), "seconds_max": round(d[-1], 7)}


def verdict(a: dict, b: dict, name_a: str, name_b: str) -> str:
    if a["seconds_median"] < b["seconds_min"]:
        return name_a
    if b["seconds_median"] < a["seconds_min"]:
        return name_b
    return "neither"


def make_log(dtype, m: int, k: int, refused: float, seed: int):
    """(log, stored offsets): m uploads of k PATCHes each, interleaved; `refused` of the records are 409s instead."""
    rng = np.random.default_rng(seed)
    n = m * k
    nbad = int(n * refused)
    late = rng.integers(0, m, nbad)
    if m >= 4:  # the 409s go to uploads that do not complete in this log: behind a DONE they would be deferred instead
        late = late // 4 * 4 + 2 + late % 2
    owners = np.concatenate((np.arange(n - nbad) % m, late))
    bad = np.concatenate((np.zeros(n - nbad, bool), np.ones(nbad, bool)))
    perm = rng.permutation(n)
    owners, bad = owners[perm], bad[perm]
    stored = np.where(np.arange(m) % 2 == 0, 0, (np.arange(m, dtype=np.uint64) + 1) * 4096).astype(np.uint64)
    # the rank of every chain PATCH within its upload, in arrival order
    chain = np.nonzero(~bad)[0]
    by_owner = chain[np.argsort(owners[chain], kind="stable")]
    sorted_owner = owners[by_owner]
    starts = np.searchsorted(sorted_owner, np.arange(m))
    rank = np.empty(n, np.uint64)
    rank[by_owner] = np.arange(len(by_owner)) - starts[sorted_owner]
    count = np.bincount(sorted_owner, minlength=m)
    log = np.zeros(n, dtype)
    log["object"], log["length"] = owners, BODY
    log["data_offset"] = (np.arange(n, dtype=np.uint64) * BODY) % (POOL - BODY)
    log["file_offset"] = stored[owners] + rank * BODY
    last = (~bad) & (rank + 1 == count[owners]) & (owners % 4 < 2) & (m >= 4)
    log["file_length"] = np.where(last, log["file_offset"] + BODY, np.uint64(UNKNOWN))
    log["file_offset"][bad] = stored[owners[bad]] + np.uint64(BODY * (k + 5) + 1)
    log["file_length"][bad] = UNKNOWN
    return log, stored


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "patches", "bench.json"))
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of the wall-clock paths")
    ap.add_argument("--seconds", type=float, default=0.3, help="device-timed work of each call")
    ap.add_argument("--shapes", default="65536x4,262144x4,4096x64,1048576x1,1x1048576")
    args = ap.parse_args()

    import torch

    from efes_amd import _lib
    from efes_amd._lib import EXTENT_DTYPE, PATCH_ANSWER_DTYPE, PATCH_DTYPE, PATCH_OBJECT_DTYPE, Objects, ObjectsOut, Patches
    from efes_amd.batch import DeviceObjects
    from efes_amd.hashing import default_context, objects_jobs_scratch, patches_table_scratch

    L = _lib.lib()
    ctx = default_context(0)
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    logf = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    pool = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    ctx.fill_synthetic(pool.data_ptr(), POOL, 0xEFE5, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fresh = np.zeros(1, _lib.SHA1_STATE_DTYPE)
    fresh["h"] = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]

    def device_time(calls: dict, seconds: float) -> dict:
        dev = {p: [] for p in calls}
        for rep in range(20000):
            todo = [p for p in dev if rep < 2 or (sum(dev[p][1:]) < seconds and len(dev[p]) < 200)]
            if not todo:
                break
            for p in todo:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                stream.synchronize()
                e0.record(stream)
                calls[p]()
                e1.record(stream)
                stream.synchronize()
                dev[p].append(e0.elapsed_time(e1) / 1e3)
        return {p: spread(t) for p, t in dev.items()}

    results = []
    for shape in args.shapes.split(","):
        m, k = (int(x) for x in shape.split("x"))
        n = m * k
        for kind, refused in (("well_formed", 0.0), ("conflicts", 0.01)):
            log_h, stored_h = make_log(PATCH_DTYPE, m, k, refused, 0xEFE5 + n + m)
            # the host twin's outputs: the reference of the check, and the host path's arrays
            ext_h, first_h = np.empty(n, EXTENT_DTYPE), np.empty(m + 1, np.uint32)
            ans_h, obj_h = np.empty(n, PATCH_ANSWER_DTYPE), np.empty(m, PATCH_OBJECT_DTYPE)
            of_h, counts_h = np.empty(n, np.uint32), np.empty(5, np.uint32)
            st_h, cr_h = np.repeat(fresh, m), np.full(m, 0x1234ABCD, np.uint32)
            st_h["h"][:, 0] = 77  # stale, but a state a Write accepts: the restarted uploads' states are written
            host_req = Patches(log=log_h.ctypes.data, offsets=stored_h.ctypes.data, sha1=st_h.ctypes.data, crc32=cr_h.ctypes.data,
                               extents=ext_h.ctypes.data, first=first_h.ctypes.data, answers=ans_h.ctypes.data, objects=obj_h.ctypes.data,
                               patch_of=of_h.ctypes.data, counts=counts_h.ctypes.data, nobjects=m, npatches=n)
            st_in, cr_in = st_h.copy(), cr_h.copy()
            assert L.efes_patches_table_host(ctypes.byref(host_req)) == 0
            assert int(counts_h[2]) == 0 and int(counts_h[4]) == 0 and int(counts_h[1]) == int(n * refused), counts_h
            with torch.cuda.stream(stream):
                dev = {name: torch.empty(max(a.nbytes, 8), dtype=torch.uint8, device="cuda:0")
                       for name, a in (("log", log_h), ("offsets", stored_h), ("sha1", st_h), ("crc32", cr_h), ("extents", ext_h), ("first", first_h),
                                       ("answers", ans_h), ("objects", obj_h), ("patch_of", of_h), ("counts", counts_h))}
                scratch = torch.empty(max(patches_table_scratch(m, n), objects_jobs_scratch(m, n)), dtype=torch.uint8, device="cuda:0")
            dev_req = Patches(nobjects=m, npatches=n, **{name: t.data_ptr() for name, t in dev.items()})
            as_t = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1))
            log_t, stored_t, st_in_t, cr_in_t = as_t(log_h), as_t(stored_h), as_t(st_in), as_t(cr_in)
            ext_t, first_t, st_t, cr_t = as_t(ext_h), as_t(first_h), as_t(st_h), as_t(cr_h)
            put = lambda name, t: dev[name][: t.numel()].copy_(t)

            def call():
                ctx.patches_table(dev_req, scratch.data_ptr(), scratch.numel(), s)

            def path_device():
                put("log", log_t)
                put("offsets", stored_t)
                call()
                stream.synchronize()

            def path_host():
                L.efes_patches_table_host(ctypes.byref(host_req))
                put("extents", ext_t)
                put("first", first_t)
                put("sha1", st_t)
                put("crc32", cr_t)
                stream.synchronize()

            wall = {"device": [], "host": []}
            with torch.cuda.stream(stream):
                put("sha1", st_in_t)
                put("crc32", cr_in_t)
                path_device()  # the check: the device against the twin, byte for byte
                for name, a in (("extents", ext_h), ("first", first_h), ("answers", ans_h), ("objects", obj_h), ("patch_of", of_h),
                                ("counts", counts_h), ("sha1", st_h), ("crc32", cr_h)):
                    assert dev[name][: a.nbytes].cpu().numpy().tobytes() == a.tobytes(), (shape, kind, name)
                for rep in range(args.reps + 1):
                    for p, fn in (("device", path_device), ("host", path_host)):
                        st_h[:], cr_h[:] = st_in, cr_in  # the twin resets the states it is given
                        stream.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        wall[p].append(time.perf_counter() - t0)
                # the builder and the walk behind the call
                sums = torch.empty(24 * n, dtype=torch.uint8, device="cuda:0")
                status = torch.empty(n, dtype=torch.int32, device="cuda:0")
                jobs = torch.empty(56 * n, dtype=torch.uint8, device="cuda:0")
                table = Objects(data=pool.data_ptr(), extents=dev["extents"].data_ptr(), first=dev["first"].data_ptr(), sha1=dev["sha1"].data_ptr(),
                                crc32=dev["crc32"].data_ptr(), sums=sums.data_ptr(), status=status.data_ptr(), nobjects=m, nextents=n, flags=0,
                                copy_align=256)
                out = ObjectsOut(jobs=jobs.data_ptr())
                calls = {"call": call, "builder": lambda: ctx.objects_jobs(table, out, scratch.data_ptr(), scratch.numel(), s)}
                if m > 1:
                    walk_scratch = torch.empty(max(int(L.efes_hash_chain_scratch(n)), 16), dtype=torch.uint8, device="cuda:0")
                    calls["walk"] = lambda: ctx.hash_chain_wide(jobs.data_ptr(), n, None, walk_scratch.data_ptr(), walk_scratch.numel(), s)
                device = device_time(calls, args.seconds)
                assert m == 1 or (status.cpu().numpy() == 0).all()
            row = {"shape": shape, "log": kind, "uploads": m, "patches": n, "verdicts": counts_h.tolist(), "log_bytes": 40 * n + 8 * m,
                   "table_bytes": 16 * n + 4 * (m + 1) + 108 * m, "wall": {p: spread(t) for p, t in wall.items()}, "device": device}
            row["wins"] = verdict(row["wall"]["device"], row["wall"]["host"], "device", "host")
            row["device_median_over_host_min"] = round(row["wall"]["device"]["seconds_median"] / row["wall"]["host"]["seconds_min"], 4)
            results.append(row)
            for f in (sys.stdout, logf):
                print(json.dumps(row), file=f, flush=True)
            del dev, scratch, sums, status, jobs
            torch.cuda.empty_cache()
        if m == 1:
            continue
        # what the zero-length slots cost: 10 % refused PATCHes in the table, against the table compacted on the host
        log_h, stored_h = make_log(PATCH_DTYPE, m, k, 0.10, 0xC0FFEE + n + m)
        with torch.cuda.stream(stream):
            full = DeviceObjects.from_patches(pool.data_ptr(), log_h, stored_h, sha1=True, walk="wide", ctx=ctx)
            stream.synchronize()
            ext = full._table_ext.cpu().numpy()
            first = full._table_first.cpu().numpy().view(np.uint32).astype(np.int64)
            answers = full.patch_answers_host()
            keep = np.ones(n, bool)
            keep[answers["slot"][(answers["verdict"] != 0) & (answers["verdict"] != 3)]] = False
            before = np.concatenate(([0], np.cumsum(keep)))
            compact = DeviceObjects.from_table(pool.data_ptr(), torch.from_numpy(ext[keep].copy()).to("cuda:0"),
                                               torch.from_numpy(before[first].astype(np.uint32).view(np.int32)).to("cuda:0"), sha1=True,
                                               walk="wide", fresh=False, states=full.states_host().copy(),
                                               crcs=full.crcs.cpu().numpy().view(np.uint32)[:m].copy(), ctx=ctx)
            stream.synchronize()

            def rerun(o):
                o.reset()
                o.submit()

            device = device_time({"walk_with_refused_slots": lambda: rerun(full), "walk_compacted": lambda: rerun(compact)}, args.seconds)
            rerun(full)
            rerun(compact)
            stream.synchronize()
            assert all(a == b for a, b in zip(full.sha1_hex(), compact.sha1_hex()) if b is not None), shape  # None: every PATCH of the upload was refused
        row = {"shape": shape, "log": "refused_10_percent", "uploads": m, "patches": n, "slots_compacted": int(keep.sum()), "device": device,
               "wins": verdict(device["walk_with_refused_slots"], device["walk_compacted"], "with_refused_slots", "compacted"),
               "refused_median_over_compacted_median": round(device["walk_with_refused_slots"]["seconds_median"] / device["walk_compacted"]["seconds_median"], 4)}
        results.append(row)
        for f in (sys.stdout, logf):
            print(json.dumps(row), file=f, flush=True)
        del full, compact
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_patches.py", "device": torch.cuda.get_device_name(0), "build_id": L.efes_build_id().decode(),
           "wall_reps": args.reps, "seconds_per_device_path": args.seconds, "body_bytes": BODY,
           "checks": "every output of the device call and the reset states equal the host twin's byte for byte; the walk's statuses are EFES_OK; the compacted table gives the same digests",
           "rows": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    logf.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
