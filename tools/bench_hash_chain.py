"""Chained SHA-1 + CRC-32 jobs against what a caller had before, in one GPU run: writes
profiles/hash_chain_group/bench.json and bench.log beside it (profiles/hash_chain/ holds the run from
before the grouped walk, paths (a) to (c)).

    python tools/bench_hash_chain.py [--out PATH] [--seconds 1.0] [--shapes 0,1,2,3,4,5,6]

Synthetic bytes in a 4 GiB pool (well past the 256 MiB Infinity Cache), fused jobs, every repetition from
NewSha1() / NewCRC32IEEE().  The paths alternate in this process, each warmed once and then repeated until
its device-event-timed work reaches --seconds:
  (a) chain -- one efes_hash_chain call over all extents, one state pair per object;
  (b) steps -- what a caller does without it: one efes_hash_submit (AUTO) per extent step on one stream,
      with one job per object that still has an extent;
  (c) steps-deep -- the same launches forced to EFES_MODE_DEEP;
  (d) group -- one efes_hash_chain_mode call at the mode efes_hash_chain_auto_mode gives for the object
      count (EFES_MODE_DEEP up to one object per SIMD: then the wave walk's launches, a second sample of (a));
  (e) group4 -- the 4096-object shape only: the same call forced to EFES_MODE_GROUP4, so that the choice of
      G is seen and not assumed.
Shapes: 1024 objects x 16 extents x 256 KiB (a 4 MiB PATCH in staging chunks); 1024 x 128 x 32 KiB
(io.Copy-sized Writes); a seeded ragged set, 1024 objects of 1-64 extents of 4 KiB-1 MiB, longest object
first; 4096 x 16 x 64 KiB (more chains than SIMDs); 1024 x 4 MiB with no job flagged, where (b) and (c) are
one efes_hash_submit(AUTO) / efes_hash_submit_mode(DEEP) of the same array; 16 384 x 4 x 64 KiB; and a
seeded ragged set of 4096 objects of 1-16 extents of 4 KiB-256 KiB, longest object first.
Before any rate is printed every path's status must be EFES_OK, the objects' 24-byte sums of all paths
must be equal, and two objects per shape must match hashlib and zlib.

    python tools/bench_hash_chain.py --checkpoints [--out PATH] [--seconds 1.0] [--shapes 0,1,2,3,4]

is the checkpoint leg (main_checkpoints below): efes_hash_chain_checkpoints with a record on every extent
against efes_hash_chain_mode and against the steps with a device copy of the states after each; it writes
profiles/hash_chain_ckpt/bench.json and bench.log, with the engine clock of each path's last repetition.

    python tools/bench_hash_chain.py --wide [--checkpoints] [--out PATH] [--seconds 1.0] [--shapes 0,1,2,3,4,5]

is the wide-walk leg (main_wide below): efes_hash_chain_wide against efes_hash_chain_mode at
efes_hash_chain_auto_mode's mode and against the steps, on many small objects; with --checkpoints also the
three ways to a record on every extent, in the same run.  It writes profiles/hash_chain_wide/bench.json and
bench.log.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POOL = 4 << 30


def equal_shape(nobj: int, next_: int, size: int):
    """Per object: [(offset, length)] -- the pool cut into consecutive extents, object after object."""
    assert nobj * next_ * size == POOL
    return [[((i * next_ + k) * size, size) for k in range(next_)] for i in range(nobj)]


def ragged_shape(seed: int = 0x4A66ED, nobj: int = 1024, max_extents: int = 64, max_size: int = 1 << 20):
    """nobj objects of 1-max_extents extents of 4 KiB-max_size at seeded 4 KiB-aligned pool offsets, longest
    object first."""
    rng = np.random.default_rng(seed)
    objects = []
    for _ in range(nobj):
        k = int(rng.integers(1, max_extents + 1))
        lens = rng.integers(4 << 10, max_size + 1, size=k)
        offs = rng.integers(0, (POOL - max_size) >> 12, size=k) << 12
        objects.append([(int(o), int(n)) for o, n in zip(offs, lens)])
    objects.sort(key=lambda o: -sum(n for _, n in o))
    return objects


SHAPES = [("1024 objects x 16 extents x 256 KiB", lambda: equal_shape(1024, 16, 256 << 10)),
          ("1024 objects x 128 extents x 32 KiB", lambda: equal_shape(1024, 128, 32 << 10)),
          ("ragged: 1024 objects x 1-64 extents x 4 KiB-1 MiB, longest first", ragged_shape),
          ("4096 objects x 16 extents x 64 KiB", lambda: equal_shape(4096, 16, 64 << 10)),
          ("1024 x 4 MiB, unflagged", lambda: equal_shape(1024, 1, 4 << 20)),
          ("16384 objects x 4 extents x 64 KiB", lambda: equal_shape(16384, 4, 64 << 10)),
          ("ragged: 4096 objects x 1-16 extents x 4 KiB-256 KiB, longest first",
           lambda: ragged_shape(0x4A66EE, 4096, 16, 256 << 10))]
FORCED_GROUP4 = {3}  # shapes with column (e)


def stats(total: int, dev: list[float]) -> dict:
    """Repetition 0 is the warm-up."""
    d = sorted(dev[1:])
    med = d[len(d) // 2]
    return {"reps": len(d), "device_seconds_median": round(med, 6), "device_seconds_min": round(d[0], 6),
            "device_seconds_max": round(d[-1], 6), "spread_min_max_over_median": [round(d[0] / med, 4), round(d[-1] / med, 4)],
            "GiB_per_s": round(total / med / 2**30, 2)}


def packed_shape(nobj: int, next_: int, size: int):
    """equal_shape over the front of the pool only."""
    return [[((i * next_ + k) * size, size) for k in range(next_)] for i in range(nobj)]


CKPT_SHAPES = [SHAPES[2], SHAPES[0], SHAPES[3], SHAPES[6],
               ("4096 objects x 64 extents x 4 KiB", lambda: packed_shape(4096, 64, 4 << 10))]


def main_checkpoints(args) -> int:
    """The --checkpoints leg: the resumable state after EVERY extent, three ways, on the shapes of CKPT_SHAPES.
      ckpt         -- one efes_hash_chain_checkpoints call, a record per extent, at the mode
                      efes_hash_chain_auto_mode gives for the object count;
      mode         -- the same array through efes_hash_chain_mode at that mode: the call without the records;
      steps-copies -- what a caller does today for the same records: one efes_hash_submit (AUTO) per extent
                      step and one device copy of all states (SHA-1 and CRC, one buffer) after each step;
      text         -- separately, efes_checkpoints_marshal_text over all records of the shape.
    Before any rate: every status EFES_OK, the sums of all paths equal, every record of ckpt equal to the state
    steps-copies copied after that extent's step, two objects equal to hashlib and zlib, and the texts of the
    first and last record equal to the host codecs."""
    import ctypes

    import torch

    from bench_crc_batch import Probe
    from efes_amd import _lib
    from efes_amd.hashing import default_context, hash_chain_auto_mode, hash_chain_scratch

    FIN, INIT, CHAIN = _lib.EFES_JOB_FINALIZE, _lib.EFES_JOB_INIT, _lib.EFES_JOB_CHAIN
    REC, TEXT = _lib.CHECKPOINT_DTYPE.itemsize, _lib.CHECKPOINT_TEXT_BYTES
    mode_name = {v: k for k, v in {"DEEP": _lib.MODE_DEEP, **{"GROUP%d" % g: m for g, m in _lib.MODE_GROUP.items()}}.items()}
    chosen = {int(x) for x in args.shapes.split(",")}
    ctx = default_context(0)
    probe = Probe()
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    buf = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    results = []
    for si, (name, make) in enumerate(CKPT_SHAPES):
        if si not in chosen:
            continue
        objects = make()
        nobj = len(objects)
        counts = np.array([len(o) for o in objects], dtype=np.int64)
        n, steps = int(counts.sum()), int(counts.max())
        total = int(sum(m for o in objects for _, m in o))
        owner = np.repeat(np.arange(nobj, dtype=np.uint64), counts)
        step = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
        ext = np.array([e for o in objects for e in o], dtype=np.uint64).reshape(n, 2)
        last = step == counts[owner.astype(np.int64)] - 1
        mode = hash_chain_auto_mode(nobj, ctx)
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(buf.data_ptr(), POOL, 0x5A1C + si, s)
            # one buffer per path: nobj SHA-1 states, then nobj CRCs, so that steps-copies copies both at once
            res = {p: dict(st=torch.zeros(nobj * 108, dtype=torch.uint8, device="cuda:0"),
                           sums=torch.zeros(nobj * 24, dtype=torch.uint8, device="cuda:0"),
                           status=torch.full((n,), -99, dtype=torch.int32, device="cuda:0")) for p in ("ckpt", "mode", "steps-copies")}

            def job_array(r, order, chained):
                j = np.zeros(n, dtype=_lib.JOB_DTYPE)
                j["data"] = np.uint64(buf.data_ptr()) + ext[:, 0]
                j["length"] = ext[:, 1]
                j["sha1"] = np.uint64(r["st"].data_ptr()) + owner * np.uint64(104)
                j["crc32"] = np.uint64(r["st"].data_ptr() + 104 * nobj) + owner * np.uint64(4)
                j["sum"] = np.uint64(r["sums"].data_ptr()) + owner * np.uint64(24)  # FINALIZE on the last extent only
                j["status"] = np.uint64(r["status"].data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4)
                j["flags"] = np.where(step == 0, INIT, CHAIN if chained else 0).astype(np.uint32) | np.where(last, FIN, 0).astype(np.uint32)
                return torch.from_numpy(j[order].view(np.uint8).copy()).to("cuda:0")

            by_step = np.argsort(step, kind="stable")
            first_of_step = np.searchsorted(step[by_step], np.arange(steps + 1))
            jobs = {"ckpt": job_array(res["ckpt"], np.arange(n), True), "mode": job_array(res["mode"], np.arange(n), True),
                    "steps-copies": job_array(res["steps-copies"], by_step, False)}
            scratch = torch.empty(hash_chain_scratch(n), dtype=torch.uint8, device="cuda:0")
            recs = torch.zeros(n * REC, dtype=torch.uint8, device="cuda:0")
            at = np.uint64(recs.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(REC)
            ptrs = torch.from_numpy(at.view(np.uint8).copy()).to("cuda:0")
            snaps = torch.zeros((steps, nobj * 108), dtype=torch.uint8, device="cuda:0")
            text = torch.zeros(n * TEXT, dtype=torch.uint8, device="cuda:0")
        stream.synchronize()

        def run_ckpt():
            ctx.hash_chain_checkpoints(jobs["ckpt"].data_ptr(), n, ptrs.data_ptr(), scratch.data_ptr(), scratch.numel(), s, mode)

        def run_mode():
            ctx.hash_chain_mode(jobs["mode"].data_ptr(), n, scratch.data_ptr(), scratch.numel(), s, mode)

        def run_steps_copies():
            base = jobs["steps-copies"].data_ptr()
            for k in range(steps):
                a, b = int(first_of_step[k]), int(first_of_step[k + 1])
                ctx.submit(base + 56 * a, b - a, s, _lib.MODE_AUTO)
                snaps[k].copy_(res["steps-copies"]["st"], non_blocking=True)

        def run_text():
            ctx.checkpoints_marshal_text(recs.data_ptr(), n, text.data_ptr(), s)

        paths = {"ckpt": run_ckpt, "mode": run_mode, "steps-copies": run_steps_copies, "text": run_text}
        dev, clock = {p: [] for p in paths}, {}
        with torch.cuda.stream(stream):
            for rep in range(20000):
                todo = [p for p in paths if rep < 2 or sum(dev[p][1:]) < (args.seconds if p != "text" else args.seconds / 10)]
                if not todo:
                    break
                for p in todo:  # alternating; repetition 0 is the warm-up
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    marked = probe.mark(s, 0)
                    e0.record(stream)
                    paths[p]()
                    e1.record(stream)
                    marked = marked and probe.mark(s, 1)
                    stream.synchronize()
                    dev[p].append(e0.elapsed_time(e1) / 1e3)
                    if marked:
                        clock[p] = probe.read()
        stream.synchronize()
        # ---- correctness before any rate
        sums = {p: res[p]["sums"].cpu().numpy().reshape(nobj, 24) for p in res}
        for p in res:
            assert (res[p]["status"].cpu().numpy() == 0).all(), (name, p)
            assert (sums[p] == sums["ckpt"]).all(), (name, p)
            assert (res[p]["st"].cpu().numpy() == res["ckpt"]["st"].cpu().numpy()).all(), (name, p)
        for i in {0, nobj - 1}:
            data = b"".join(bytes(buf[a:a + m].cpu().numpy()) for a, m in objects[i])
            assert bytes(sums["ckpt"][i]) == hashlib.sha1(data).digest() + zlib.crc32(data).to_bytes(4, "big"), (name, i)
        got = recs.cpu().numpy().view(_lib.CHECKPOINT_DTYPE)
        snap = snaps.cpu().numpy()
        own = owner.astype(np.int64)
        want_sha = snap[:, :104 * nobj].reshape(steps, nobj, 104)[step, own].copy().view(_lib.SHA1_STATE_DTYPE).reshape(n)
        want_crc = snap[:, 104 * nobj:].copy().view(np.uint32).reshape(steps, nobj)[step, own]
        for f in ("h", "x", "nx", "len"):
            assert (got["sha1"][f] == want_sha[f]).all(), (name, "record", f)
        assert (got["crc"] == want_crc).all() and (got["_pad"] == 0).all() and (got["sha1"]["_pad"] == 0).all(), (name, "record")
        texts = text.cpu().numpy().reshape(n, TEXT)
        for j in (0, n - 1):
            raw = got[j].tobytes()
            a, b = ctypes.create_string_buffer(200), ctypes.create_string_buffer(8)
            _lib.lib().efes_sha1_state_marshal_text(ctypes.byref(_lib.Sha1State.from_buffer_copy(raw[:104])), a)
            _lib.lib().efes_crc32_state_marshal_text(ctypes.byref(_lib.Crc32State.from_buffer_copy(raw[104:108])), b)
            assert bytes(texts[j]) == a.raw + b.raw, (name, "text", j)
        row = {"shape": name, "objects": nobj, "jobs": n, "extent_steps": steps, "bytes": total, "mode": mode_name[mode],
               "record_bytes": n * REC, "text_bytes": n * TEXT,
               "paths": {p: {**stats(total, dev[p]), "engine_mhz": clock.get(p)} for p in paths}}
        del row["paths"]["text"]["GiB_per_s"]  # not a pass over the data
        c = row["paths"]["ckpt"]["device_seconds_median"]
        row["ckpt_over_mode"] = round(c / row["paths"]["mode"]["device_seconds_median"], 4)
        row["ckpt_over_steps_copies"] = round(c / row["paths"]["steps-copies"]["device_seconds_median"], 4)
        row["mode_spread_min_max_over_median"] = row["paths"]["mode"]["spread_min_max_over_median"]
        row["text_over_ckpt"] = round(row["paths"]["text"]["device_seconds_median"] / c, 4)
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
    out = {"tool": "tools/bench_hash_chain.py --checkpoints", "device": torch.cuda.get_device_name(0),
           "build_id": _lib.lib().efes_build_id().decode(), "pool_bytes": POOL, "seconds_per_path": args.seconds,
           "checks": "every status EFES_OK; all paths' sums and final states equal; every record equal to the state copied after "
                     "that extent's step; two objects per shape equal hashlib and zlib; two texts per shape equal the host codecs",
           "shapes": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


WIDE_SHAPES = [SHAPES[5],
               ("32768 objects x 4 extents x 32 KiB", lambda: equal_shape(32768, 4, 32 << 10)),
               ("65536 objects x 4 extents x 16 KiB", lambda: equal_shape(65536, 4, 16 << 10)),
               ("262144 objects x 4 extents x 4 KiB", lambda: equal_shape(262144, 4, 4 << 10)),
               CKPT_SHAPES[4],
               ("ragged: 65536 objects x 1-8 extents x 4 KiB-64 KiB, longest first",
                lambda: ragged_shape(0x4A66EF, 65536, 8, 64 << 10))]


def main_wide(args) -> int:
    """The --wide leg, on the shapes of WIDE_SHAPES:
      wide         -- (a) one efes_hash_chain_wide call, ckpt_device NULL;
      mode         -- (b) efes_hash_chain_mode at the mode efes_hash_chain_auto_mode gives for the object count;
      steps        -- (c) one efes_hash_submit (AUTO) per extent step, one job per object that still has an extent;
    and with --checkpoints, in the same run:
      wide-ckpt    -- (a') efes_hash_chain_wide with a record on every extent;
      ckpt         -- (b') efes_hash_chain_checkpoints at that mode;
      steps-copies -- (c') the steps plus one device copy of all states after each step.
    Before any rate: every status EFES_OK, all paths' sums and final states equal, the records of wide-ckpt equal
    to those of ckpt and to the states steps-copies copied, two objects per shape equal to hashlib and zlib."""
    import torch

    from bench_crc_batch import Probe
    from efes_amd import _lib
    from efes_amd.hashing import default_context, hash_chain_auto_mode, hash_chain_scratch

    FIN, INIT, CHAIN = _lib.EFES_JOB_FINALIZE, _lib.EFES_JOB_INIT, _lib.EFES_JOB_CHAIN
    REC = _lib.CHECKPOINT_DTYPE.itemsize
    mode_name = {v: k for k, v in {"DEEP": _lib.MODE_DEEP, **{"GROUP%d" % g: m for g, m in _lib.MODE_GROUP.items()}}.items()}
    chosen = {int(x) for x in args.shapes.split(",")}
    names = ["wide", "mode", "steps"] + (["wide-ckpt", "ckpt", "steps-copies"] if args.checkpoints else [])
    ctx = default_context(0)
    probe = Probe()
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    buf = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    results = []
    for si, (name, make) in enumerate(WIDE_SHAPES):
        if si not in chosen:
            continue
        objects = make()
        nobj = len(objects)
        counts = np.array([len(o) for o in objects], dtype=np.int64)
        n, steps = int(counts.sum()), int(counts.max())
        owner = np.repeat(np.arange(nobj, dtype=np.uint64), counts)
        own = owner.astype(np.int64)
        step = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
        ext = np.array([e for o in objects for e in o], dtype=np.uint64).reshape(n, 2)
        total = int(ext[:, 1].sum())
        last = step == counts[own] - 1
        mode = hash_chain_auto_mode(nobj, ctx)
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(buf.data_ptr(), POOL, 0x5A1C + 16 + si, s)
            res = {p: dict(st=torch.zeros(nobj * 108, dtype=torch.uint8, device="cuda:0"),
                           sums=torch.zeros(nobj * 24, dtype=torch.uint8, device="cuda:0"),
                           status=torch.full((n,), -99, dtype=torch.int32, device="cuda:0")) for p in names}

            def job_array(r, order, chained):
                j = np.zeros(n, dtype=_lib.JOB_DTYPE)
                j["data"] = np.uint64(buf.data_ptr()) + ext[:, 0]
                j["length"] = ext[:, 1]
                j["sha1"] = np.uint64(r["st"].data_ptr()) + owner * np.uint64(104)
                j["crc32"] = np.uint64(r["st"].data_ptr() + 104 * nobj) + owner * np.uint64(4)
                j["sum"] = np.uint64(r["sums"].data_ptr()) + owner * np.uint64(24)  # FINALIZE on the last extent only
                j["status"] = np.uint64(r["status"].data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4)
                j["flags"] = np.where(step == 0, INIT, CHAIN if chained else 0).astype(np.uint32) | np.where(last, FIN, 0).astype(np.uint32)
                return torch.from_numpy(j[order].view(np.uint8).copy()).to("cuda:0")

            by_step = np.argsort(step, kind="stable")
            first_of_step = np.searchsorted(step[by_step], np.arange(steps + 1))
            jobs = {p: job_array(res[p], by_step if p.startswith("steps") else np.arange(n), not p.startswith("steps")) for p in names}
            scratch = torch.empty(hash_chain_scratch(n), dtype=torch.uint8, device="cuda:0")
            if args.checkpoints:
                recs = {p: torch.zeros(n * REC, dtype=torch.uint8, device="cuda:0") for p in ("wide-ckpt", "ckpt")}
                ptrs = {p: torch.from_numpy((np.uint64(recs[p].data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(REC))
                                            .view(np.uint8).copy()).to("cuda:0") for p in recs}
                snaps = torch.zeros((steps, nobj * 108), dtype=torch.uint8, device="cuda:0")
        stream.synchronize()

        def run_steps(p, copies):
            base = jobs[p].data_ptr()
            for k in range(steps):
                a, b = int(first_of_step[k]), int(first_of_step[k + 1])
                ctx.submit(base + 56 * a, b - a, s, _lib.MODE_AUTO)
                if copies:
                    snaps[k].copy_(res[p]["st"], non_blocking=True)

        paths = {"wide": lambda: ctx.hash_chain_wide(jobs["wide"].data_ptr(), n, None, scratch.data_ptr(), scratch.numel(), s),
                 "mode": lambda: ctx.hash_chain_mode(jobs["mode"].data_ptr(), n, scratch.data_ptr(), scratch.numel(), s, mode),
                 "steps": lambda: run_steps("steps", False)}
        if args.checkpoints:
            paths["wide-ckpt"] = lambda: ctx.hash_chain_wide(jobs["wide-ckpt"].data_ptr(), n, ptrs["wide-ckpt"].data_ptr(),
                                                             scratch.data_ptr(), scratch.numel(), s)
            paths["ckpt"] = lambda: ctx.hash_chain_checkpoints(jobs["ckpt"].data_ptr(), n, ptrs["ckpt"].data_ptr(), scratch.data_ptr(),
                                                               scratch.numel(), s, mode)
            paths["steps-copies"] = lambda: run_steps("steps-copies", True)
        dev, clock = {p: [] for p in paths}, {}
        with torch.cuda.stream(stream):
            for rep in range(20000):
                todo = [p for p in paths if rep < 2 or sum(dev[p][1:]) < args.seconds]
                if not todo:
                    break
                for p in todo:  # alternating; repetition 0 is the warm-up
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    stream.synchronize()
                    marked = probe.mark(s, 0)
                    e0.record(stream)
                    paths[p]()
                    e1.record(stream)
                    marked = marked and probe.mark(s, 1)
                    stream.synchronize()
                    dev[p].append(e0.elapsed_time(e1) / 1e3)
                    if marked:
                        clock[p] = probe.read()
        stream.synchronize()
        # ---- correctness before any rate
        sums = {p: res[p]["sums"].cpu().numpy().reshape(nobj, 24) for p in paths}
        st0 = res["mode"]["st"].cpu().numpy()
        for p in paths:
            assert (res[p]["status"].cpu().numpy() == 0).all(), (name, p)
            assert (sums[p] == sums["mode"]).all(), (name, p)
            assert (res[p]["st"].cpu().numpy() == st0).all(), (name, p)
        for i in {0, nobj - 1}:
            data = b"".join(bytes(buf[a:a + m].cpu().numpy()) for a, m in objects[i])
            assert bytes(sums["wide"][i]) == hashlib.sha1(data).digest() + zlib.crc32(data).to_bytes(4, "big"), (name, i)
        if args.checkpoints:
            got = recs["wide-ckpt"].cpu().numpy()
            assert (got == recs["ckpt"].cpu().numpy()).all(), (name, "records")
            got = got.view(_lib.CHECKPOINT_DTYPE)
            snap = snaps.cpu().numpy()
            want_sha = snap[:, :104 * nobj].reshape(steps, nobj, 104)[step, own].copy().view(_lib.SHA1_STATE_DTYPE).reshape(n)
            want_crc = snap[:, 104 * nobj:].copy().view(np.uint32).reshape(steps, nobj)[step, own]
            for f in ("h", "x", "nx", "len"):
                assert (got["sha1"][f] == want_sha[f]).all(), (name, "record", f)
            assert (got["crc"] == want_crc).all() and (got["_pad"] == 0).all() and (got["sha1"]["_pad"] == 0).all(), (name, "record")
        row = {"shape": name, "objects": nobj, "jobs": n, "extent_steps": steps, "bytes": total, "mode": mode_name[mode],
               "paths": {p: {**stats(total, dev[p]), "engine_mhz": clock.get(p)} for p in paths}}
        P = row["paths"]
        row["wide_over_mode"] = round(P["wide"]["device_seconds_median"] / P["mode"]["device_seconds_median"], 4)
        row["wide_over_steps"] = round(P["wide"]["device_seconds_median"] / P["steps"]["device_seconds_median"], 4)
        row["wide_median_below_mode_min"] = P["wide"]["device_seconds_median"] < P["mode"]["device_seconds_min"]
        if args.checkpoints:
            row["wide_ckpt_over_ckpt"] = round(P["wide-ckpt"]["device_seconds_median"] / P["ckpt"]["device_seconds_median"], 4)
            row["wide_ckpt_over_steps_copies"] = round(P["wide-ckpt"]["device_seconds_median"] / P["steps-copies"]["device_seconds_median"], 4)
            row["wide_ckpt_over_wide"] = round(P["wide-ckpt"]["device_seconds_median"] / P["wide"]["device_seconds_median"], 4)
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
        del res, jobs, scratch
        if args.checkpoints:
            del recs, ptrs, snaps
    out = {"tool": "tools/bench_hash_chain.py --wide" + (" --checkpoints" if args.checkpoints else ""),
           "device": torch.cuda.get_device_name(0), "build_id": _lib.lib().efes_build_id().decode(), "pool_bytes": POOL,
           "seconds_per_path": args.seconds,
           "checks": "every status EFES_OK; all paths' sums and final states equal; the wide walk's records equal to "
                     "efes_hash_chain_checkpoints' and to the states copied after each step; two objects per shape equal hashlib and zlib",
           "shapes": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seconds", type=float, default=1.0, help="device-timed work per path and shape")
    ap.add_argument("--shapes", default=None)
    ap.add_argument("--checkpoints", action="store_true",
                    help="the checkpoint leg (efes_hash_chain_checkpoints): writes profiles/hash_chain_ckpt/bench.json")
    ap.add_argument("--wide", action="store_true",
                    help="the wide-walk leg (efes_hash_chain_wide): writes profiles/hash_chain_wide/bench.json")
    args = ap.parse_args()
    if args.wide:
        args.out = args.out or os.path.join(ROOT, "profiles", "hash_chain_wide", "bench.json")
        args.shapes = args.shapes or "0,1,2,3,4,5"
        return main_wide(args)
    if args.checkpoints:
        args.out = args.out or os.path.join(ROOT, "profiles", "hash_chain_ckpt", "bench.json")
        args.shapes = args.shapes or "0,1,2,3,4"
        return main_checkpoints(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "hash_chain_group", "bench.json")
    args.shapes = args.shapes or "0,1,2,3,4,5,6"
    chosen = {int(x) for x in args.shapes.split(",")}

    import torch

    from efes_amd import _lib
    from efes_amd.hashing import default_context, hash_chain_auto_mode, hash_chain_scratch

    FIN, INIT, CHAIN = _lib.EFES_JOB_FINALIZE, _lib.EFES_JOB_INIT, _lib.EFES_JOB_CHAIN
    ctx = default_context(0)
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    buf = torch.empty(POOL, dtype=torch.uint8, device="cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    results = []
    for si, (name, make) in enumerate(SHAPES):
        if si not in chosen:
            continue
        objects = make()
        nobj = len(objects)
        counts = np.array([len(o) for o in objects], dtype=np.int64)
        n, steps = int(counts.sum()), int(counts.max())
        total = int(sum(m for o in objects for _, m in o))
        owner = np.repeat(np.arange(nobj, dtype=np.uint64), counts)
        step = np.concatenate([np.arange(c, dtype=np.int64) for c in counts])
        ext = np.array([e for o in objects for e in o], dtype=np.uint64).reshape(n, 2)
        last = step == counts[owner.astype(np.int64)] - 1
        auto = hash_chain_auto_mode(nobj, ctx)
        group_paths = {"group": auto, **({"group4": _lib.MODE_GROUP[4]} if si in FORCED_GROUP4 else {})}
        with torch.cuda.stream(stream):
            ctx.fill_synthetic(buf.data_ptr(), POOL, 0x5A1C + si, s)
            res = {p: dict(states=torch.zeros(nobj * 104, dtype=torch.uint8, device="cuda:0"),
                           crcs=torch.zeros(nobj, dtype=torch.int32, device="cuda:0"),
                           sums=torch.zeros(nobj * 24, dtype=torch.uint8, device="cuda:0"),
                           status=torch.full((n,), -99, dtype=torch.int32, device="cuda:0")) for p in ("chain", "steps", "steps-deep", *group_paths)}

            def job_array(r, order, chained):
                j = np.zeros(n, dtype=_lib.JOB_DTYPE)
                j["data"] = np.uint64(buf.data_ptr()) + ext[:, 0]
                j["length"] = ext[:, 1]
                j["sha1"] = np.uint64(r["states"].data_ptr()) + owner * np.uint64(104)
                j["crc32"] = np.uint64(r["crcs"].data_ptr()) + owner * np.uint64(4)
                j["sum"] = np.uint64(r["sums"].data_ptr()) + owner * np.uint64(24)  # FINALIZE on the last extent only
                j["status"] = np.uint64(r["status"].data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4)
                j["flags"] = np.where(step == 0, INIT, CHAIN if chained else 0).astype(np.uint32) | np.where(last, FIN, 0).astype(np.uint32)
                return torch.from_numpy(j[order].view(np.uint8).copy()).to("cuda:0")

            by_step = np.argsort(step, kind="stable")  # step after step, the objects in their order within each
            first_of_step = np.searchsorted(step[by_step], np.arange(steps + 1))
            chain_jobs = job_array(res["chain"], np.arange(n), True)
            group_jobs = {p: job_array(res[p], np.arange(n), True) for p in group_paths}
            step_jobs = {p: job_array(res[p], by_step, False) for p in ("steps", "steps-deep")}
            scratch = torch.empty(hash_chain_scratch(n), dtype=torch.uint8, device="cuda:0")
        stream.synchronize()

        def run_chain():
            ctx.hash_chain(chain_jobs.data_ptr(), n, scratch.data_ptr(), scratch.numel(), s)

        def run_group(p):
            ctx.hash_chain_mode(group_jobs[p].data_ptr(), n, scratch.data_ptr(), scratch.numel(), s, group_paths[p])

        def run_steps(p, mode):
            base = step_jobs[p].data_ptr()
            for k in range(steps):
                a, b = int(first_of_step[k]), int(first_of_step[k + 1])
                ctx.submit(base + 56 * a, b - a, s, mode)

        paths = {"chain": run_chain, "steps": lambda: run_steps("steps", _lib.MODE_AUTO),
                 "steps-deep": lambda: run_steps("steps-deep", _lib.MODE_DEEP),
                 **{p: (lambda p=p: run_group(p)) for p in group_paths}}
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
        stream.synchronize()
        # ---- correctness before any rate
        sums = {p: res[p]["sums"].cpu().numpy().reshape(nobj, 24) for p in paths}
        for p in paths:
            assert (res[p]["status"].cpu().numpy() == 0).all(), (name, p)
            assert (sums[p] == sums["chain"]).all(), (name, p, np.nonzero((sums[p] != sums["chain"]).any(axis=1))[0][:5])
            assert (res[p]["crcs"].cpu().numpy() == res["chain"]["crcs"].cpu().numpy()).all(), (name, p)
        for i in {0, nobj - 1}:
            data = b"".join(bytes(buf[a:a + m].cpu().numpy()) for a, m in objects[i])
            want = hashlib.sha1(data).digest() + zlib.crc32(data).to_bytes(4, "big")
            assert bytes(sums["chain"][i]) == want, (name, i)
        row = {"shape": name, "objects": nobj, "jobs": n, "extent_steps": steps, "bytes": total,
               "longest_object_bytes": int(max(sum(m for _, m in o) for o in objects)),
               "group_mode": {v: k for k, v in {"DEEP": _lib.MODE_DEEP, **{"GROUP%d" % g: m for g, m in _lib.MODE_GROUP.items()}}.items()}[auto],
               "paths": {p: stats(total, dev[p]) for p in paths}}
        a = row["paths"]["chain"]["device_seconds_median"]
        row["chain_over_steps"] = round(a / row["paths"]["steps"]["device_seconds_median"], 4)
        row["chain_over_steps_deep"] = round(a / row["paths"]["steps-deep"]["device_seconds_median"], 4)
        for p in group_paths:
            d = row["paths"][p]["device_seconds_median"]
            row[p + "_over_chain"] = round(d / a, 4)
            row[p + "_over_steps"] = round(d / row["paths"]["steps"]["device_seconds_median"], 4)
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
    out = {"tool": "tools/bench_hash_chain.py", "device": torch.cuda.get_device_name(0), "build_id": _lib.lib().efes_build_id().decode(),
           "pool_bytes": POOL, "seconds_per_path": args.seconds,
           "checks": "every status EFES_OK; all paths' object sums and CRC states equal; two objects per shape equal hashlib and zlib",
           "shapes": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
