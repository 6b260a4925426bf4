"""Copy with CRC (efes_crc32_copy) against what a caller had before, in one GPU run: writes
profiles/crc_copy/bench.json and bench.log beside it.

    python tools/bench_crc_copy.py [--out PATH] [--seconds 1.0] [--shapes 0,1,2,3,4]

A 4 GiB synthetic source and a 4 GiB destination per shape (well past the 256 MiB Infinity Cache), the
paths alternating in this process, each warmed once and then repeated until its device-event-timed work
reaches --seconds.
  shape 0: 16 x 256 MiB, unflagged, source and destination 16-byte aligned;
  shape 1: 64 objects x 64 extents x 1 MiB, the objects' extents interleaved in the source (extent e of
           object o sits at slot e * nobj + o) and each object contiguous in the destination: the gather is a
           transpose;
  shape 2: 1024 objects x 64 extents x 64 KiB, laid out the same way;
  shapes 3 and 4: shape 1 with every destination displaced by 1 byte and by 8 bytes (relative misalignment).
Paths:
  (a) copy_crc   -- one efes_crc32_copy call;
  (b) copy+chain -- the best single-launch copy a caller can issue (one dst.copy_(src) for shape 0, one
                    strided copy_ of the transposed view for the others, in the widest elements the
                    destination's alignment allows: 16 bytes, 8 bytes at + 8, single bytes at + 1), then
                    efes_crc32_chain over the source, both on one stream and timed together;
  (c) chain      -- efes_crc32_chain alone;
  (d) copy       -- the copy of (b) alone.
Before any rate is printed the destination of (a) must equal that of (b), the object CRCs of (a), (b) and (c)
must be equal, and two objects per shape must match zlib over the destination of (a).
Reported per shape: (a)/(b) beside (b)'s own min-max spread, whether the median of (a) lies below the minimum
of (b) (the bar for the aligned shapes 0-2; the displaced shapes are recorded only), (a)/(d), and the bytes
moved (read + written) per second by (a).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POOL = 4 << 30
SLACK = 256  # room behind the destination for the displaced shapes
SHAPES = [("16 x 256 MiB, unflagged", 16, 1, 256 << 20, 0),
          ("64 objects x 64 extents x 1 MiB, transposed", 64, 64, 1 << 20, 0),
          ("1024 objects x 64 extents x 64 KiB, transposed", 1024, 64, 64 << 10, 0),
          ("64 objects x 64 extents x 1 MiB, transposed, destination + 1 byte", 64, 64, 1 << 20, 1),
          ("64 objects x 64 extents x 1 MiB, transposed, destination + 8 bytes", 64, 64, 1 << 20, 8)]
PATHS = ("copy_crc", "copy+chain", "chain", "copy")


def stats(dev: list[float]) -> dict:
    """Repetition 0 is the warm-up."""
    d = sorted(dev[1:])
    return {"reps": len(d), "device_seconds_median": round(d[len(d) // 2], 6), "device_seconds_min": round(d[0], 6),
            "device_seconds_max": round(d[-1], 6)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc_copy", "bench.json"))
    ap.add_argument("--seconds", type=float, default=1.0, help="device-timed work per path and shape")
    ap.add_argument("--shapes", default="0,1,2,3,4", help="which of the five shapes to run")
    args = ap.parse_args()
    chosen = {int(x) for x in args.shapes.split(",")}

    import torch

    from efes_amd import _lib
    from efes_amd.hashing import crc32_chain_scratch, crc32_copy_scratch, default_context

    ctx = default_context(0)
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    src = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    dst = {p: torch.empty(POOL + SLACK, dtype=torch.uint8, device="cuda:0") for p in ("copy_crc", "copy+chain")}
    assert all(t.data_ptr() % 16 == 0 for t in (src, *dst.values()))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    results = []
    for si, (name, nobj, next_, size, disp) in enumerate(SHAPES):
        if si not in chosen:
            continue
        n = nobj * next_
        assert n * size == POOL and disp < SLACK
        idx = np.arange(n, dtype=np.uint64)  # job order: object-major, an object's extents in byte order
        owner, e = idx // np.uint64(next_), idx % np.uint64(next_)
        slot = e * np.uint64(nobj) + owner  # where the extent sits in the source
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(src.data_ptr(), POOL, 0xC09E + si, s)
            for t in dst.values():
                t.fill_(0xEE)
            obj = {p: torch.zeros(nobj, dtype=torch.int32, device="cuda:0") for p in PATHS[:3]}
            status = {p: torch.full((n,), -99, dtype=torch.int32, device="cuda:0") for p in PATHS[:3]}
            flags = np.where(e == 0, _lib.EFES_JOB_INIT, _lib.EFES_JOB_CHAIN).astype(np.uint32)  # every repetition starts fresh

            def job_array(p):
                j = np.zeros(n, dtype=_lib.JOB_DTYPE)
                j["data"] = np.uint64(src.data_ptr()) + slot * np.uint64(size)
                j["length"] = size
                j["crc32"] = np.uint64(obj[p].data_ptr()) + owner * np.uint64(4)
                j["status"] = np.uint64(status[p].data_ptr()) + idx * np.uint64(4)
                j["flags"] = flags
                return torch.from_numpy(j.view(np.uint8).copy()).to("cuda:0")

            jobs = {p: job_array(p) for p in PATHS[:3]}
            ptrs = np.uint64(dst["copy_crc"].data_ptr() + disp) + idx * np.uint64(size)
            ptrs = torch.from_numpy(ptrs.view(np.int64).copy()).to("cuda:0")
            scratch = torch.empty(max(crc32_copy_scratch(n), crc32_chain_scratch(n)), dtype=torch.uint8, device="cuda:0")
            # the plain copy: source viewed [extent][object][bytes], destination [object][extent][bytes]
            # in the widest elements the displacement allows (16 bytes, 8 bytes, single bytes)
            wide = {0: torch.complex128, 8: torch.int64}.get(disp % 16, torch.uint8)
            w = torch.empty(0, dtype=wide).element_size()
            src_view = src.view(wide).view(next_, nobj, size // w).transpose(0, 1)
            dst_view = dst["copy+chain"][disp:disp + POOL].view(wide).view(nobj, next_, size // w)
        stream.synchronize()

        def run_copy_crc():
            ctx.crc32_copy(jobs["copy_crc"].data_ptr(), ptrs.data_ptr(), n, scratch.data_ptr(), scratch.numel(), s)

        def run_copy():
            dst_view.copy_(src_view)

        def run_chain(p="chain"):
            ctx.crc32_chain(jobs[p].data_ptr(), n, scratch.data_ptr(), scratch.numel(), s)

        def run_copy_chain():
            run_copy()
            run_chain("copy+chain")

        paths = {"copy_crc": run_copy_crc, "copy+chain": run_copy_chain, "chain": run_chain, "copy": run_copy}
        dev = {p: [] for p in paths}
        with torch.cuda.stream(stream):
            for rep in range(20000):
                todo = [p for p in paths if rep < 2 or sum(dev[p][1:]) < args.seconds]
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
            # ---- correctness before any rate
            same = torch.equal(dst["copy_crc"], dst["copy+chain"])
        stream.synchronize()
        assert same, (name, "the destinations of (a) and (b) differ")
        got = {p: obj[p].cpu().numpy().view(np.uint32).copy() for p in obj}
        for p in obj:
            assert (got[p] == got["copy_crc"]).all(), (name, p, np.nonzero(got[p] != got["copy_crc"])[0][:5])
            assert (status[p].cpu().numpy() == 0).all(), (name, p)
        edges = torch.cat([dst["copy_crc"][:disp], dst["copy_crc"][disp + POOL:]]).cpu().numpy()
        assert (edges == 0xEE).all(), (name, "bytes outside the destination were written")
        m = next_ * size
        for i in {0, nobj - 1}:
            a = disp + i * m
            assert zlib.crc32(dst["copy_crc"][a:a + m].cpu().numpy()) == int(got["copy_crc"][i]), (name, i)
        row = {"shape": name, "objects": nobj, "extents_per_object": next_, "jobs": n, "bytes": POOL,
               "destination_displacement": disp, "plain_copy_element_bytes": w, "paths": {p: stats(dev[p]) for p in paths}}
        a, b, d = (row["paths"][p] for p in ("copy_crc", "copy+chain", "copy"))
        a["moved_GB_per_s"] = round(2 * POOL / a["device_seconds_median"] / 1e9, 1)  # read + written
        d["moved_GB_per_s"] = round(2 * POOL / d["device_seconds_median"] / 1e9, 1)
        row["paths"]["chain"]["read_GB_per_s"] = round(POOL / row["paths"]["chain"]["device_seconds_median"] / 1e9, 1)
        row["a_over_b"] = round(a["device_seconds_median"] / b["device_seconds_median"], 4)
        row["b_spread_min_max_over_median"] = [round(b["device_seconds_min"] / b["device_seconds_median"], 4),
                                               round(b["device_seconds_max"] / b["device_seconds_median"], 4)]
        row["a_median_below_b_min"] = a["device_seconds_median"] < b["device_seconds_min"]
        row["gated"] = disp == 0
        row["a_over_d"] = round(a["device_seconds_median"] / d["device_seconds_median"], 4)
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
    out = {"tool": "tools/bench_crc_copy.py", "device": torch.cuda.get_device_name(0), "build_id": _lib.lib().efes_build_id().decode(),
           "pool_bytes": POOL, "seconds_per_path": args.seconds,
           "checks": "destinations of (a) and (b) equal; object CRCs of (a), (b), (c) equal; two objects per shape equal zlib over the destination of (a)",
           "shapes": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
