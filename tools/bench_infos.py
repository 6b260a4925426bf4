"""Object infos on the device (efes_infos_unmarshal_text, efes_infos_marshal_text) against their host twins and against
the per-object codecs through ctypes, in one GPU run: writes profiles/infos/bench.json and bench.log beside it.

    python tools/bench_infos.py [--out PATH] [--reps 9] [--seconds 0.3] [--counts 4096,32768,65536,262144,1048576]

The record counts are the object counts of the builder's shapes (profiles/objects_jobs/bench.json) and the largest
count a table takes.  The states are random bytes, their texts the host twin's, re-cased at random, 1 % of them spoiled
in one character.  Per count, alternating in this process (repetition 0 is the warm-up; the device buffers and the
host arrays exist beforehand, so no path pays for an allocation):
  unmarshal:
    call    -- efes_infos_unmarshal_text alone, between two events; device time.  Also with EVERY text invalid, where
               every workgroup takes its two atomics on the counters.
    device  -- the texts from host memory to the device (208 bytes per object), the call, a synchronise; wall time.
    host    -- efes_infos_unmarshal_text_host, then the states and CRCs to the device (108 bytes per object), a
               synchronise; wall time.
    loop    -- what the library offered before: efes_sha1_state_unmarshal_text and efes_crc32_state_unmarshal_text per
               object through ctypes into the same arrays, the same upload and synchronise; wall time; only at 65 536
               records or fewer, three repetitions.
  marshal:
    call    -- efes_infos_marshal_text alone; device time.
    device  -- the call, the texts to the host (208 bytes per object); wall time.
    host    -- the states and CRCs to the host (108 bytes per object), efes_infos_marshal_text_host; wall time.
A path "wins" where its median is below the other's minimum.  Before any figure is reported the device's states, CRCs,
statuses, counts and texts equal the host twin's byte for byte."""
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

T = 208
LOOP_MAX = 65536


def spread(t: list[float]) -> dict:
    d = sorted(t[1:])
    return {"reps": len(d), "seconds_median": round(d[len(d) // 2], 7), "seconds_min": round(d[0], 7), "seconds_max": round(d[-1], 7)}


def verdict(a: dict, b: dict, name_a: str, name_b: str) -> str:
    if a["seconds_median"] < b["seconds_min"]:
        return name_a
    if b["seconds_median"] < a["seconds_min"]:
        return name_b
    return "neither"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infos", "bench.json"))
    ap.add_argument("--reps", type=int, default=9, help="timed repetitions of the wall-clock paths")
    ap.add_argument("--seconds", type=float, default=0.3, help="device-timed work of each call")
    ap.add_argument("--counts", default="4096,32768,65536,262144,1048576")
    args = ap.parse_args()

    import torch

    from efes_amd import _lib
    from efes_amd._lib import Crc32State, Infos, Sha1State
    from efes_amd.hashing import default_context

    L = _lib.lib()
    ctx = default_context(0)
    stream = torch.cuda.Stream(device="cuda:0")
    s = stream.cuda_stream
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    log = open(os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.log"), "w")
    results = []
    for n in [int(x) for x in args.counts.split(",")]:
        rng = np.random.default_rng(0xEFE5 + n)
        states_h = rng.integers(0, 256, 104 * n, dtype=np.uint8)
        crcs_h = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        text_h = np.empty(T * n, np.uint8)
        host_req = lambda text, st, cr, status=None, counts=None: Infos(
            text=text.ctypes.data, sha1=st.ctypes.data, crc32=cr.ctypes.data, status=None if status is None else status.ctypes.data,
            counts=None if counts is None else counts.ctypes.data, n=n)
        assert L.efes_infos_marshal_text_host(ctypes.byref(host_req(text_h, states_h, crcs_h))) == 0
        rows = text_h.reshape(n, T)
        letters = (rows >= ord("a")) & (rows <= ord("f")) & (rng.integers(0, 2, rows.shape) == 1)
        rows[letters] -= 32  # mixed case
        spoiled = np.sort(rng.choice(n, max(1, n // 100), replace=False))
        rows[spoiled, rng.integers(0, T, len(spoiled))] = ord("g")
        # what the host twin leaves: the reference of the checks, and the host path's outputs
        st_out, cr_out = np.empty(104 * n, np.uint8), np.empty(n, np.uint32)
        status_out, counts_out = np.empty(n, np.int32), np.empty(2, np.uint32)
        unmarshal_req = host_req(text_h, st_out, cr_out, status_out, counts_out)
        assert L.efes_infos_unmarshal_text_host(ctypes.byref(unmarshal_req)) == 0
        assert counts_out.tolist() == [n - len(spoiled), len(spoiled)]
        text_out = np.empty(T * n, np.uint8)
        marshal_req = host_req(text_out, st_out, cr_out)
        with torch.cuda.stream(stream):
            text_d = torch.empty(T * n, dtype=torch.uint8, device="cuda:0")
            st_d, cr_d = torch.empty(104 * n, dtype=torch.uint8, device="cuda:0"), torch.empty(4 * n, dtype=torch.uint8, device="cuda:0")
            status_d, counts_d = torch.empty(n, dtype=torch.int32, device="cuda:0"), torch.empty(2, dtype=torch.int32, device="cuda:0")
            back_d = torch.empty(T * n, dtype=torch.uint8, device="cuda:0")
        dev_req = Infos(text=text_d.data_ptr(), sha1=st_d.data_ptr(), crc32=cr_d.data_ptr(), status=status_d.data_ptr(),
                        counts=counts_d.data_ptr(), n=n)
        back_req = Infos(text=back_d.data_ptr(), sha1=st_d.data_ptr(), crc32=cr_d.data_ptr(), n=n)
        text_t, st_t, cr_t = torch.from_numpy(text_h), torch.from_numpy(st_out), torch.from_numpy(cr_out.view(np.uint8))
        back_t = torch.from_numpy(text_out)
        stream.synchronize()

        def unmarshal_device():
            text_d.copy_(text_t)
            ctx.infos_unmarshal_text(dev_req, s)
            stream.synchronize()

        def upload_states():
            st_d.copy_(st_t)
            cr_d.copy_(cr_t)
            stream.synchronize()

        def unmarshal_host():
            L.efes_infos_unmarshal_text_host(ctypes.byref(unmarshal_req))
            upload_states()

        def unmarshal_loop():
            st, cr = Sha1State(), Crc32State()
            sha_fn, crc_fn = L.efes_sha1_state_unmarshal_text, L.efes_crc32_state_unmarshal_text
            raw = text_h.tobytes()
            for i in range(n):
                a = sha_fn(ctypes.byref(st), raw[T * i:T * i + 200], 200)
                b = crc_fn(ctypes.byref(cr), raw[T * i + 200:T * i + T], 8)
                if a == 0 and b == 0:
                    ctypes.memmove(st_out.ctypes.data + 104 * i, ctypes.byref(st), 104)
                    cr_out[i] = cr.crc
            upload_states()

        def marshal_device():
            ctx.infos_marshal_text(back_req, s)
            back_t.copy_(back_d)
            stream.synchronize()

        def marshal_host():
            st_t.copy_(st_d)
            cr_t.copy_(cr_d)
            stream.synchronize()
            L.efes_infos_marshal_text_host(ctypes.byref(marshal_req))

        want = (st_out.copy(), cr_out.copy(), status_out.copy())
        wall = {"unmarshal_device": [], "unmarshal_host": [], "marshal_device": [], "marshal_host": []}
        paths = {"unmarshal_device": unmarshal_device, "unmarshal_host": unmarshal_host, "marshal_device": marshal_device, "marshal_host": marshal_host}
        with torch.cuda.stream(stream):
            unmarshal_device()  # the checks: the device against the twin, byte for byte
            assert st_d.cpu().numpy().tobytes() == want[0].tobytes() and cr_d.cpu().numpy().tobytes() == want[1].tobytes(), n
            assert status_d.cpu().numpy().tobytes() == want[2].tobytes() and counts_d.cpu().numpy().view(np.uint32).tolist() == counts_out.tolist(), n
            marshal_host()
            host_text = text_out.copy()
            text_out[:] = 0
            marshal_device()
            assert text_out.tobytes() == host_text.tobytes(), n
            for rep in range(args.reps + 1):
                for p, fn in paths.items():
                    stream.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    wall[p].append(time.perf_counter() - t0)
            loop = []
            if n <= LOOP_MAX:
                for rep in range(4):
                    stream.synchronize()
                    t0 = time.perf_counter()
                    unmarshal_loop()
                    loop.append(time.perf_counter() - t0)
                assert st_out.tobytes() == want[0].tobytes() and cr_out.tobytes() == want[1].tobytes()
            dev = {"unmarshal_call": [], "marshal_call": [], "unmarshal_call_all_invalid": []}
            broken_d = torch.full((T * n,), ord("g"), dtype=torch.uint8, device="cuda:0")  # every workgroup takes its two atomics
            broken_req = Infos(text=broken_d.data_ptr(), sha1=st_d.data_ptr(), crc32=cr_d.data_ptr(), status=status_d.data_ptr(),
                               counts=counts_d.data_ptr(), n=n)
            calls = {"unmarshal_call": lambda: ctx.infos_unmarshal_text(dev_req, s), "marshal_call": lambda: ctx.infos_marshal_text(back_req, s),
                     "unmarshal_call_all_invalid": lambda: ctx.infos_unmarshal_text(broken_req, s)}
            text_d.copy_(text_t)
            for rep in range(20000):
                todo = [p for p in dev if rep < 2 or sum(dev[p][1:]) < args.seconds]
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
            assert counts_d.cpu().numpy().view(np.uint32).tolist() in ([n - len(spoiled), len(spoiled)], [0, n])
            del broken_d
        row = {"records": n, "spoiled": len(spoiled), "text_bytes": T * n, "state_bytes": 108 * n,
               "wall": {p: spread(t) for p, t in wall.items()}, "device": {p: spread(t) for p, t in dev.items()}}
        if loop:
            row["wall"]["unmarshal_ctypes_loop"] = spread(loop)
        for kind in ("unmarshal", "marshal"):
            d, h = row["wall"][kind + "_device"], row["wall"][kind + "_host"]
            row[kind + "_wins"] = verdict(d, h, "device", "host")
            row[kind + "_device_median_over_host_min"] = round(d["seconds_median"] / h["seconds_min"], 4)
            moved = (T + 108) * n  # read plus written by the call
            row[kind + "_call_TB_per_s"] = round(moved / row["device"][kind + "_call"]["seconds_median"] / 1e12, 3)
        results.append(row)
        for f in (sys.stdout, log):
            print(json.dumps(row), file=f, flush=True)
        del text_d, st_d, cr_d, status_d, counts_d, back_d
        torch.cuda.empty_cache()
    out = {"tool": "tools/bench_infos.py", "device": torch.cuda.get_device_name(0), "build_id": L.efes_build_id().decode(),
           "wall_reps": args.reps, "seconds_per_device_path": args.seconds, "ctypes_loop_up_to": LOOP_MAX,
           "checks": "the device's states, CRCs, statuses, counts and texts equal the host twins' byte for byte; the ctypes loop's states too",
           "counts": results}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    log.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
