"""The wide chain walk with copy (efes_hash_chain_wide_copy) against what a caller had before, in one GPU run:
writes profiles/hash_chain_wide_copy/bench.json and bench.log beside it.

    python tools/bench_hash_chain_copy.py [--out PATH] [--seconds 1.0] [--shapes 0,1,2,3] [--paths a,b,c,d,e,a+1,a+8]
                                          [--parent PARENT.json]

Fused jobs (SHA-1 + CRC-32, FINALIZE on each object's last extent) over a 4 GiB synthetic pool, every object
gathered contiguously -- each extent behind the one before it -- at a COPY_ALIGN-aligned destination offset
(default_copy_offsets).  The shapes are the four on which the wide walk wins (profiles/hash_chain_wide/):
  shape 0: 32 768 objects x 4 extents x 32 KiB;
  shape 1: 65 536 objects x 4 extents x 16 KiB;
  shape 2: 262 144 objects x 4 extents x 4 KiB;
           in these three the objects' extents are interleaved in the pool (extent e of object o sits at slot
           e * nobj + o), so the gather is a transpose, as in tools/bench_crc_copy.py;
  shape 3: the ragged set of tools/bench_hash_chain.py --wide: 65 536 objects of 1-8 extents of 4-64 KiB at seeded
           4 KiB-aligned pool offsets, longest first (lengths of any byte count, so the extents behind an
           object's first land at odd addresses).
Paths, alternating in this process, each warmed once and then repeated until its device-event-timed work reaches
--seconds (a quarter of it for the displaced runs):
  (a) wide_copy      -- one efes_hash_chain_wide_copy call, ckpt_device NULL;
  (b) wide+copy      -- efes_hash_chain_wide, then the best single-launch copy of the same extents, on one stream
                        and timed together (the two-call path);
  (c) wide           -- efes_hash_chain_wide alone;
  (d) copy           -- that copy alone;
  (e) wide_copy-ckpt -- (a) with a record on every extent;
  a+1, a+8           -- (a) with every destination displaced by 1 byte and by 8 bytes.
The copy of (b) and (d): for the equal shapes one strided copy_ of the transposed view in 16-byte elements (the
yardstick of tools/bench_crc_copy.py) and the plain gather kernel of tools/gathercopy.hip are both timed before the
run and the faster one is taken; the ragged set has no strided view, so there it is the gather kernel.
Before any rate is reported: every status is EFES_OK; the sums and final states of (a), (e) and the displaced runs
equal (c)'s, and (e)'s records equal those of one efes_hash_chain_wide call with the same record array; the
destination of (a) equals that of (b) byte for byte, those of (e) and of the displaced runs equal it at their
displacement, and the bytes around every destination keep their fill; two objects per shape equal hashlib and zlib
over the DESTINATION of (a).
Reported per shape: (a)/(b), (a)/(c), (a)/(d), (e)/(a), the displaced runs over (a), and whether (a)'s median lies
below (b)'s minimum.  --paths c runs efes_hash_chain_wide alone (it needs nothing this call added, so the same file
runs in a tree of the parent commit); --parent merges such a run's JSON under "parent" and says per shape whether
this tree's median of (c) lies within the parent's own min-max spread.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

POOL = 4 << 30
SLACK = 256  # room in front of and behind every destination: the displaced runs, and the fill that must survive
FILL = 0xEE
NAMES = {"a": "wide_copy", "b": "wide+copy", "c": "wide", "d": "copy", "e": "wide_copy-ckpt", "a+1": "wide_copy+1",
         "a+8": "wide_copy+8"}
DISP = {"a+1": 1, "a+8": 8}


def transposed_shape(nobj: int, next_: int, size: int):
    """Per object: [(offset, length)] -- extent e of object o at pool slot e * nobj + o."""
    assert nobj * next_ * size == POOL
    return [[((e * nobj + o) * size, size) for e in range(next_)] for o in range(nobj)]


def ragged():
    from bench_hash_chain import ragged_shape
    return ragged_shape(0x4A66EF, 65536, 8, 64 << 10)


SHAPES = [("32768 objects x 4 extents x 32 KiB, transposed", lambda: transposed_shape(32768, 4, 32 << 10), (32768, 4, 32 << 10)),
          ("65536 objects x 4 extents x 16 KiB, transposed", lambda: transposed_shape(65536, 4, 16 << 10), (65536, 4, 16 << 10)),
          ("262144 objects x 4 extents x 4 KiB, transposed", lambda: transposed_shape(262144, 4, 4 << 10), (262144, 4, 4 << 10)),
          ("ragged: 65536 objects x 1-8 extents x 4 KiB-64 KiB, longest first", ragged, None)]


def stats(dev: list[float]) -> dict:
    """Repetition 0 is the warm-up."""
    d = sorted(dev[1:])
    return {"reps": len(d), "device_seconds_median": round(d[len(d) // 2], 6), "device_seconds_min": round(d[0], 6),
            "device_seconds_max": round(d[-1], 6)}


class Gather:
    """tools/gathercopy.hip through ctypes: one launch that copies n byte-granular extents."""

    def __init__(self, torch, src_ptrs: np.ndarray, lens: np.ndarray, cus: int):
        self.lib = ctypes.CDLL(os.path.join(ROOT, "tools", "libgathercopy.so"))
        self.lib.gathercopy_chunk.restype = ctypes.c_uint32
        self.lib.gathercopy_launch.restype = ctypes.c_int
        self.lib.gathercopy_launch.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
        chunk = int(self.lib.gathercopy_chunk())
        first = np.concatenate(([0], np.cumsum((lens + np.uint64(chunk - 1)) // np.uint64(chunk)))).astype(np.uint64)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).to("cuda:0")
        self.up, self.n, self.groups = up, int(lens.size), 8 * cus
        self.src, self.len, self.first = up(src_ptrs), up(lens), up(first)

    def launcher(self, dst_ptrs: np.ndarray, stream: int):
        dst = self.up(dst_ptrs)

        def run():
            rc = self.lib.gathercopy_launch(0, self.src.data_ptr(), dst.data_ptr(), self.len.data_ptr(), self.first.data_ptr(),
                                            self.n, self.groups, stream)
            assert rc == 0, rc
        run.keep = dst
        return run


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_chain_wide_copy", "bench.json"))
    ap.add_argument("--seconds", type=float, default=1.0, help="device-timed work per path and shape")
    ap.add_argument("--shapes", default="0,1,2,3")
    ap.add_argument("--paths", default="a,b,c,d,e,a+1,a+8")
    ap.add_argument("--parent", default=None, help="the JSON of a --paths c run in a tree of the parent commit, same machine")
    args = ap.parse_args()
    chosen = {int(x) for x in args.shapes.split(",")}
    want = [p for p in NAMES if p in set(args.paths.split(","))]
    full = want == list(NAMES)
    assert full or want == ["c"], "--paths: all seven, or c alone"

    import torch

    from efes_amd import _lib
    from efes_amd.batch import COPY_ALIGN, default_copy_offsets
    from efes_amd.hashing import default_context, hash_chain_scratch

    FIN, INIT, CHAIN = _lib.EFES_JOB_FINALIZE, _lib.EFES_JOB_INIT, _lib.EFES_JOB_CHAIN
    REC = _lib.CHECKPOINT_DTYPE.itemsize
    ctx = default_context(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    pool = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log" if full else "bench_c.log"), "w")
    results = []
    for si, (name, make, equal) in enumerate(SHAPES):
        if si not in chosen:
            continue
        objects = make()
        nobj = len(objects)
        counts = np.array([len(o) for o in objects], dtype=np.int64)
        n = int(counts.sum())
        owner = np.repeat(np.arange(nobj, dtype=np.uint64), counts)
        own = owner.astype(np.int64)
        step = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
        ext = np.array([e for o in objects for e in o], dtype=np.uint64).reshape(n, 2)
        total = int(ext[:, 1].sum())
        last = step == counts[own] - 1
        offsets, room = default_copy_offsets(objects)
        assert (offsets % COPY_ALIGN == 0).all()
        first_job = np.concatenate(([0], np.cumsum(counts)))[:-1]
        before = np.cumsum(ext[:, 1]) - ext[:, 1]
        within = before - before[first_job[own]]
        rel = np.asarray(offsets, dtype=np.uint64)[own] + within  # each extent behind the one before it in its object
        hashed = [p for p in want if p != "d"]
        with_dst = [p for p in want if p not in ("c", "d")]
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(pool.data_ptr(), POOL, 0x5A1C + 32 + si, s)
            res = {p: dict(st=torch.zeros(nobj * 108, dtype=torch.uint8, device="cuda:0"),
                           sums=torch.zeros(nobj * 24, dtype=torch.uint8, device="cuda:0"),
                           status=torch.full((n,), -99, dtype=torch.int32, device="cuda:0")) for p in hashed + ["c-ckpt"]}
            dst = {p: torch.full((room + 2 * SLACK,), FILL, dtype=torch.uint8, device="cuda:0") for p in with_dst}
            assert all(t.data_ptr() % COPY_ALIGN == 0 for t in dst.values())

            def job_array(r):
                j = np.zeros(n, dtype=_lib.JOB_DTYPE)
                j["data"] = np.uint64(pool.data_ptr()) + ext[:, 0]
                j["length"] = ext[:, 1]
                j["sha1"] = np.uint64(r["st"].data_ptr()) + owner * np.uint64(104)
                j["crc32"] = np.uint64(r["st"].data_ptr() + 104 * nobj) + owner * np.uint64(4)
                j["sum"] = np.uint64(r["sums"].data_ptr()) + owner * np.uint64(24)  # FINALIZE on the last extent only
                j["status"] = np.uint64(r["status"].data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4)
                j["flags"] = np.where(step == 0, INIT, CHAIN).astype(np.uint32) | np.where(last, FIN, 0).astype(np.uint32)
                return torch.from_numpy(j.view(np.uint8).copy()).to("cuda:0")

            def dst_ptrs(p):
                return np.uint64(dst[p].data_ptr() + SLACK + DISP.get(p, 0)) + rel

            up = lambda a: torch.from_numpy(a.astype(np.uint64).view(np.int64).copy()).to("cuda:0")
            jobs = {p: job_array(res[p]) for p in res}
            ptrs = {p: up(dst_ptrs(p)) for p in with_dst if p != "b"}
            scratch = torch.empty(hash_chain_scratch(n), dtype=torch.uint8, device="cuda:0")
            if full:
                recs = {p: torch.zeros(n * REC, dtype=torch.uint8, device="cuda:0") for p in ("e", "c-ckpt")}
                rptr = {p: up(np.uint64(recs[p].data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(REC)) for p in recs}
        stream.synchronize()

        def wide(p, ck=None):
            ctx.hash_chain_wide(jobs[p].data_ptr(), n, ck, scratch.data_ptr(), scratch.numel(), s)

        def wide_copy(p, ck=None):
            ctx.hash_chain_wide_copy(jobs[p].data_ptr(), n, ptrs[p].data_ptr(), ck, scratch.data_ptr(), scratch.numel(), s)

        copy_kind = None
        if full:
            # ---- the copy of (b) and (d): the faster of the candidates, timed before the run
            gather = Gather(torch, np.uint64(pool.data_ptr()) + ext[:, 0], ext[:, 1], cus)
            candidates = {"gather kernel (tools/gathercopy.hip)": gather.launcher(dst_ptrs("b"), s)}
            if equal:
                eo, ee, es = equal
                assert room == POOL and (rel == np.arange(n, dtype=np.uint64) * np.uint64(es)).all()
                src_view = pool.view(torch.complex128).view(ee, eo, es // 16).transpose(0, 1)
                dst_view = dst["b"][SLACK:SLACK + POOL].view(torch.complex128).view(eo, ee, es // 16)
                candidates["strided copy_ in 16-byte elements"] = lambda: dst_view.copy_(src_view)
            trial = {}
            with torch.cuda.stream(stream):
                for kind, f in candidates.items():
                    t = []
                    for _ in range(6):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        stream.synchronize()
                        e0.record(stream)
                        f()
                        e1.record(stream)
                        stream.synchronize()
                        t.append(e0.elapsed_time(e1) / 1e3)
                    trial[kind] = round(sorted(t[1:])[2], 6)
            copy_kind = min(trial, key=trial.get)
            run_copy = candidates[copy_kind]

        paths = {}
        if "a" in want:
            paths["a"] = lambda: wide_copy("a")
            paths["b"] = lambda: (wide("b"), run_copy())
        paths["c"] = lambda: wide("c")
        if "a" in want:
            paths["d"] = lambda: run_copy()
            paths["e"] = lambda: wide_copy("e", rptr["e"].data_ptr())
            paths["a+1"] = lambda: wide_copy("a+1")
            paths["a+8"] = lambda: wide_copy("a+8")
        dev = {p: [] for p in paths}
        with torch.cuda.stream(stream):
            for rep in range(20000):
                todo = [p for p in paths if rep < 2 or sum(dev[p][1:]) < (args.seconds / 4 if p in DISP else args.seconds)]
                if not todo:
                    break
                for p in todo:  # alternating; repetition 0 is the warm-up
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    e0.record(stream)
                    paths[p]()
                    e1.record(stream)
                    stream.synchronize()
                    dev[p].append(e0.elapsed_time(e1) / 1e3)
            if full:
                wide("c-ckpt", rptr["c-ckpt"].data_ptr())  # the records (c) gives, once, outside the timing
        stream.synchronize()
        # ---- correctness before any rate
        sums = {p: res[p]["sums"].cpu().numpy().reshape(nobj, 24) for p in res if p in hashed or full}
        st0 = res["c"]["st"].cpu().numpy()
        for p in sums:
            assert (res[p]["status"].cpu().numpy() == 0).all(), (name, p, "status")
            assert (sums[p] == sums["c"]).all(), (name, p, "sums")
            assert (res[p]["st"].cpu().numpy() == st0).all(), (name, p, "states")
        spots = sorted({0, nobj - 1})
        if full:
            assert torch.equal(recs["e"], recs["c-ckpt"]), (name, "records of (e) and of efes_hash_chain_wide differ")
            assert torch.equal(dst["a"], dst["b"]), (name, "the destinations of (a) and (b) differ")
            for p in ("e", "a+1", "a+8"):
                d = DISP.get(p, 0)
                assert torch.equal(dst[p][SLACK + d:SLACK + d + room], dst["a"][SLACK:SLACK + room]), (name, p, "destination")
                assert bool((dst[p][:SLACK + d] == FILL).all()) and bool((dst[p][SLACK + d + room:] == FILL).all()), (name, p, "fill")
            assert bool((dst["a"][:SLACK] == FILL).all()) and bool((dst["a"][SLACK + room:] == FILL).all()), (name, "fill")
            for i in spots:
                a = SLACK + int(offsets[i])
                m = int(sum(k for _, k in objects[i]))
                data = bytes(dst["a"][a:a + m].cpu().numpy())
                assert data == b"".join(bytes(pool[o:o + k].cpu().numpy()) for o, k in objects[i]), (name, i, "gathered bytes")
                assert bytes(sums["a"][i]) == hashlib.sha1(data).digest() + zlib.crc32(data).to_bytes(4, "big"), (name, i)
        else:
            for i in spots:
                data = b"".join(bytes(pool[o:o + k].cpu().numpy()) for o, k in objects[i])
                assert bytes(sums["c"][i]) == hashlib.sha1(data).digest() + zlib.crc32(data).to_bytes(4, "big"), (name, i)
        row = {"shape": name, "objects": nobj, "jobs": n, "bytes": total, "destination_bytes": int(room),
               "paths": {NAMES[p]: stats(dev[p]) for p in paths}}
        P = row["paths"]
        med = lambda p: P[NAMES[p]]["device_seconds_median"]
        P["wide"]["GiB_per_s"] = round(total / med("c") / 2**30, 2)
        if full:
            row["copy_of_b_and_d"] = copy_kind
            row["copy_candidates_seconds_median"] = trial
            P["wide_copy"]["GiB_per_s"] = round(total / med("a") / 2**30, 2)
            P["copy"]["moved_GB_per_s"] = round(2 * total / med("d") / 1e9, 1)  # read + written
            row["a_over_b"] = round(med("a") / med("b"), 4)
            row["a_over_c"] = round(med("a") / med("c"), 4)
            row["a_over_d"] = round(med("a") / med("d"), 4)
            row["e_over_a"] = round(med("e") / med("a"), 4)
            row["a_plus_1_over_a"] = round(med("a+1") / med("a"), 4)
            row["a_plus_8_over_a"] = round(med("a+8") / med("a"), 4)
            row["b_spread_min_max_over_median"] = [round(P["wide+copy"]["device_seconds_min"] / med("b"), 4),
                                                   round(P["wide+copy"]["device_seconds_max"] / med("b"), 4)]
            row["a_median_below_b_min"] = med("a") < P["wide+copy"]["device_seconds_min"]
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
        del res, jobs, scratch, dst, ptrs, paths
        if full:
            del recs, rptr, gather, candidates, run_copy
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_hash_chain_copy.py" + ("" if full else " --paths c"), "device": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().efes_build_id().decode(), "pool_bytes": POOL, "seconds_per_path": args.seconds,
           "checks": ("every status EFES_OK; sums and final states of (a), (e) and the displaced runs equal (c)'s; (e)'s records equal "
                      "efes_hash_chain_wide's; the destination of (a) equals (b)'s, (e)'s and the displaced runs' equal it, the fill "
                      "around every destination intact; two objects per shape equal hashlib and zlib over the destination of (a)")
           if full else "every status EFES_OK; two objects per shape equal hashlib and zlib",
           "shapes": results}
    if args.parent:
        parent = json.load(open(args.parent))
        by = {r["shape"]: r for r in parent["shapes"]}
        rows = []
        for r in results:
            pw, tw = by[r["shape"]]["paths"]["wide"], r["paths"]["wide"]
            rows.append({"shape": r["shape"], "parent": pw, "this_tree_median": tw["device_seconds_median"],
                         "this_over_parent": round(tw["device_seconds_median"] / pw["device_seconds_median"], 4),
                         "this_median_within_parent_min_max": pw["device_seconds_min"] <= tw["device_seconds_median"] <= pw["device_seconds_max"]})
        out["parent"] = {"what": "(c) efes_hash_chain_wide alone, this tool with --paths c in a tree of the parent commit, same machine",
                         "build_id": parent["build_id"], "device": parent["device"], "shapes": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
