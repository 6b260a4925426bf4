"""CRC-only batches, three ways, in one GPU run: writes profiles/crc_batch/bench.json.

    python tools/bench_crc_batch.py [--out PATH] [--seconds 1.0]

Per shape (4 GiB of synthetic bytes, well past the 256 MiB Infinity Cache) the same CRC-only job array
runs, alternating in this process, through
  (a) batch  -- efes_crc32_batch;
  (b) submit -- efes_hash_submit(MODE_AUTO), the path CRC-only jobs had before (the baseline);
  (c) span   -- efes_crc32_span per object, for shapes of at most 64 jobs;
each warmed once and then timed with device events until it has run for --seconds.  Before any rate
is printed every path's CRCs must be equal and two jobs per shape must match zlib.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POOL = 4 << 30
SPEC_BYTES_PER_S = 8e12  # HBM3E, spec
MIXED_JOBS = 4096


def shapes():
    from efes_amd.chunksize import mixed_geometry

    out = []
    for n, size in [(1, 4 << 30), (16, 256 << 20), (64, 64 << 20), (1024, 4 << 20), (65536, 64 << 10)]:
        out.append((f"{n} x {size >> 10} KiB", np.full(n, size, dtype=np.uint64), np.arange(n, dtype=np.uint64) * np.uint64(size)))
    sizes, offs = mixed_geometry(MIXED_JOBS, POOL, 7)
    out.append((f"mixed_geometry({MIXED_JOBS}), 64 KiB - 64 MiB", sizes, offs))
    return out


class Probe:
    """The engine clock over a region, from bench.py's probe library when it has been built."""

    def __init__(self):
        path = os.path.join(ROOT, "tools", "libclockprobe.so")
        self.lib = None
        if os.path.exists(path):
            try:
                self.lib = ctypes.CDLL(path)
                self.lib.clockprobe_mark.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
                self.lib.clockprobe_read.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                                     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
            except (OSError, AttributeError):
                self.lib = None

    def mark(self, stream: int, which: int) -> bool:
        return self.lib is not None and self.lib.clockprobe_mark(0, stream, which) == 0

    def read(self):
        mhz, sec, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        if self.lib is not None and self.lib.clockprobe_read(0, ctypes.byref(mhz), ctypes.byref(sec), ctypes.byref(n)) == 0:
            return round(mhz.value, 1)
        return None


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc_batch", "bench.json"))
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per path and shape")
    args = ap.parse_args()

    import torch

    from efes_amd import _lib
    from efes_amd.hashing import crc32_batch_scratch, default_context

    ctx = default_context(0)
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    probe = Probe()
    buf = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    results = []
    for si, (name, sizes, offs) in enumerate(shapes()):
        n = int(sizes.size)
        total = int(sizes.sum())
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(buf.data_ptr(), POOL, 0xC4C + si, s)
            crcs = {p: torch.zeros(n, dtype=torch.int32, device="cuda:0") for p in ("batch", "submit", "span")}
            status = torch.full((n,), -99, dtype=torch.int32, device="cuda:0")
            jobs = {}
            for p in ("batch", "submit"):
                j = np.zeros(n, dtype=_lib.JOB_DTYPE)
                j["data"] = np.uint64(buf.data_ptr()) + offs
                j["length"] = sizes
                j["crc32"] = np.uint64(crcs[p].data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4)
                j["status"] = np.uint64(status.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4)
                j["flags"] = _lib.EFES_JOB_INIT  # every repetition starts from NewCRC32IEEE()
                jobs[p] = torch.from_numpy(j.view(np.uint8).copy()).to("cuda:0")
            scratch = torch.empty(crc32_batch_scratch(n), dtype=torch.uint8, device="cuda:0")
        stream.synchronize()

        def run_batch():
            ctx.crc32_batch(jobs["batch"].data_ptr(), n, scratch.data_ptr(), scratch.numel(), s)

        def run_submit():
            ctx.submit(jobs["submit"].data_ptr(), n, s, _lib.MODE_AUTO)

        def run_span():
            crcs["span"].zero_()
            for k in range(n):
                ctx.crc32_span(buf.data_ptr() + int(offs[k]), int(sizes[k]), crcs["span"].data_ptr() + 4 * k, s)

        paths = {"batch": run_batch, "submit": run_submit}
        if n <= 64:
            paths["span"] = run_span
        times = {p: [] for p in paths}
        clock = {}
        with torch.cuda.stream(stream):
            for rep in range(20000):
                todo = [p for p in paths if rep < 2 or sum(times[p][1:]) < args.seconds]
                if not todo:
                    break
                for p in todo:  # alternating; repetition 0 is the warm-up
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    marked = probe.mark(s, 0)
                    e0.record(stream)
                    paths[p]()
                    e1.record(stream)
                    marked = marked and probe.mark(s, 1)
                    stream.synchronize()
                    times[p].append(e0.elapsed_time(e1) / 1e3)
                    if marked:
                        clock[p] = probe.read()
                    if rep == 0 and times[p][0] >= args.seconds:
                        times[p].append(times[p][0])  # one run already is the timed work: count it, run once more
        stream.synchronize()
        # ---- correctness before any rate
        got = {p: crcs[p].cpu().numpy().view(np.uint32) for p in paths}
        for p in paths:
            assert (got[p] == got["batch"]).all(), (name, p, np.nonzero(got[p] != got["batch"])[0][:5])
        assert (status.cpu().numpy() == 0).all(), name
        for k in {0, n - 1} if n > 1 else {0, 0}:
            crc, a, m = 0, int(offs[k]), int(sizes[k])
            for at in range(a, a + m, 1 << 30):
                crc = zlib.crc32(buf[at:min(a + m, at + (1 << 30))].cpu().numpy(), crc)
            assert crc == int(got["batch"][k]), (name, k, hex(crc), hex(int(got["batch"][k])))
        row = {"shape": name, "jobs": n, "bytes": total, "paths": {}}
        for p in paths:
            t = sorted(times[p][1:])
            med = t[len(t) // 2]
            row["paths"][p] = {"reps": len(t), "seconds_median": round(med, 6), "seconds_min": round(t[0], 6),
                               "GB_per_s": round(total / med / 1e9, 1), "share_of_8TBps": round(total / med / SPEC_BYTES_PER_S, 4),
                               "engine_mhz": clock.get(p)}
        row["batch_over_submit"] = round(row["paths"]["submit"]["seconds_median"] / row["paths"]["batch"]["seconds_median"], 2)
        if "span" in row["paths"]:
            row["batch_over_span"] = round(row["paths"]["span"]["seconds_median"] / row["paths"]["batch"]["seconds_median"], 3)
        results.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "tools/bench_crc_batch.py", "device": torch.cuda.get_device_name(0), "build_id": _lib.lib().efes_build_id().decode(),
           "pool_bytes": POOL, "tile_bytes": _lib.EFES_CRC_BATCH_TILE, "seconds_per_path": args.seconds,
           "checks": "all paths' CRCs equal; two jobs per shape equal zlib", "shapes": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
