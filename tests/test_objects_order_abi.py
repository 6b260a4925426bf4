"""Object order (efes_objects_order, efes_objects_jobs_ordered, their scratch sizes and host twins) without a GPU:
the six symbols and their declarations, the ABI version they leave alone, the scratch sizes, the argument errors of
the device calls that need no device, and DeviceObjects(order=...)'s argument check."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")
WANT = {"efes_objects_order_scratch": ["nobjects", "nextents"],
        "efes_objects_order": ["ctx", "in", "order_device", "scratch_device", "scratch_bytes", "stream"],
        "efes_objects_order_host": ["in", "order"],
        "efes_objects_jobs_ordered_scratch": ["nobjects", "nextents"],
        "efes_objects_jobs_ordered": ["ctx", "in", "out", "order_device", "job_first_device", "scratch_device", "scratch_bytes",
                                      "stream"],
        "efes_objects_jobs_ordered_host": ["in", "out", "order", "job_first"]}
TOP = 1 << 20


def test_symbols_are_declared_and_exported(efes_lib):
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want in WANT.items():
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in efes_hash.h"
        args = [a.strip().split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
        assert args == want, (name, args)
        assert getattr(efes_lib.lib(), name)
        assert len(efes_lib.SIGNATURES[name][1]) == len(args)
    from efes_amd import hashing
    assert hasattr(hashing.Context, "objects_order") and hasattr(hashing.Context, "objects_jobs_ordered")
    assert hashing.objects_order_scratch and hashing.objects_jobs_ordered_scratch
    assert hashing.objects_order_host and hashing.objects_jobs_ordered_host


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8
    assert re.search(r"#define\s+EFES_ABI_VERSION\s+8\b", open(HEADER).read())


@pytest.mark.parametrize("which", ["objects_order_scratch", "objects_jobs_ordered_scratch"])
def test_scratch_sizes(efes_lib, which):
    """0 for refused counts and never 0 otherwise; 16-byte multiples that grow with either count."""
    from efes_amd import hashing
    scratch = getattr(hashing, which)
    assert scratch(TOP + 1, 1) == 0 and scratch(1, TOP + 1) == 0 and scratch(TOP + 1, TOP + 1) == 0
    counts = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2051, 4096, 4097, 65536, TOP - 1, TOP]
    for m in counts:
        sizes = [scratch(m, n) for n in counts]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes), (m, sizes)
    for n in counts:
        sizes = [scratch(m, n) for m in counts]
        assert sizes == sorted(sizes), (n, sizes)
    assert scratch(TOP, TOP) < 48 << 20
    if which == "objects_jobs_ordered_scratch":  # the builder's two scans and the scan of the counts, 64-bit words each
        assert all(scratch(m, n) >= 8 * (n + 1) + 16 * (m + 1) for m in counts for n in counts)
        assert all(scratch(m, n) >= hashing.objects_jobs_scratch(m, n) for m in counts for n in counts)
    else:  # the scan of the lengths, two buffers of (key, value) pairs
        assert all(scratch(m, n) >= 8 * (n + 1) + 24 * m for m in counts for n in counts)


def _table(efes_lib, n=4, m=2):
    keep = dict(ext=np.zeros((n, 2), np.uint64), first=np.array([0, 1, n][: m + 1], np.uint32),
                order=np.full(m + 2, 0xA5A5A5A5, np.uint32), jobs=np.zeros(n, efes_lib.JOB_DTYPE),
                job_first=np.full(m + 3, 0xA5A5A5A5, np.uint32))
    t = efes_lib.Objects(data=0x1000, extents=keep["ext"].ctypes.data, first=keep["first"].ctypes.data, sha1=0x2000, crc32=0x3000,
                         sums=0x4000, status=0x5000, nobjects=m, nextents=n, flags=1)
    return t, keep


def test_device_calls_check_their_arguments_before_the_device(efes_lib):
    """A NULL context is EFES_ERR_ARG on its own; so is every table error, without any device; nothing is written."""
    L = efes_lib.lib()
    t, keep = _table(efes_lib)
    before = {k: v.copy() for k, v in keep.items()}
    o = efes_lib.ObjectsOut(jobs=keep["jobs"].ctypes.data)
    order, jf = keep["order"].ctypes.data, keep["job_first"].ctypes.data
    assert L.efes_objects_order(None, ctypes.byref(t), order, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_order(None, None, None, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_jobs_ordered(None, ctypes.byref(t), ctypes.byref(o), order, jf, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_jobs_ordered(None, None, None, None, None, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert all((keep[k] == before[k]).all() for k in keep)


@pytest.mark.parametrize("order", ["Table", "longest", "", None, 1, [2, 1, 0], np.arange(3, dtype=np.uint32)])
def test_device_objects_rejects_unknown_orders(efes_lib, order):
    """Raised from the argument alone, before any context or device is touched."""
    from efes_amd.batch import DeviceObjects
    with pytest.raises(ValueError, match="order"):
        DeviceObjects(0x1000, [[(0, 16)]], build="device", order=order)


def test_an_order_needs_the_device_build(efes_lib):
    from efes_amd.batch import DeviceObjects
    with pytest.raises(ValueError, match='build="device"'):
        DeviceObjects(0x1000, [[(0, 16)]], order="longest_first")
    with pytest.raises(ValueError, match='build="device"'):
        DeviceObjects(0x1000, [[(0, 16)]], build="host", order="longest_first")
