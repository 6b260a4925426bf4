"""Object tables (efes_objects_jobs, efes_objects_jobs_scratch, efes_objects_jobs_host) without a GPU: the symbols
and their declarations, the struct layouts against the ctypes mirrors, the ABI version they leave alone, every
argument error that needs no device, the scratch size, and DeviceObjects(build=...)'s argument check.

efes_objects is 96 bytes: the ten pointers and four 32-bit words that the interface names (10 x 8 + 4 x 4); the
figure is taken from the fields, through the C compiler."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")
NAMES = ["efes_objects_jobs_scratch", "efes_objects_jobs", "efes_objects_jobs_host"]
OBJECT_FIELDS = ["data", "extents", "first", "sha1", "crc32", "sums", "status", "ckpt", "copy_to", "copy_offsets",
                 "nobjects", "nextents", "flags", "copy_align"]
OUT_FIELDS = ["jobs", "dst", "ckpt", "layout"]


def test_symbols_are_declared_and_exported(efes_lib):
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    want = {"efes_objects_jobs_scratch": ["nobjects", "nextents"],
            "efes_objects_jobs": ["ctx", "in", "out", "scratch_device", "scratch_bytes", "stream"],
            "efes_objects_jobs_host": ["in", "out"]}
    for name in NAMES:
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in efes_hash.h"
        args = [a.strip().split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
        assert args == want[name], (name, args)
        assert getattr(efes_lib.lib(), name)
        assert len(efes_lib.SIGNATURES[name][1]) == len(args)
    from efes_amd import hashing
    assert hasattr(hashing.Context, "objects_jobs") and hashing.objects_jobs_scratch and hashing.objects_jobs_host


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8
    assert re.search(r"#define\s+EFES_ABI_VERSION\s+8\b", open(HEADER).read())


def test_struct_layouts_match_header(tmp_path, efes_lib):
    prog = tmp_path / "objects.c"
    fields = "".join(f', offsetof(efes_objects, {f})' for f in OBJECT_FIELDS) + "".join(f', offsetof(efes_objects_out, {f})' for f in OUT_FIELDS)
    prog.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "efes_hash.h"
int main(void) {
  size_t v[] = {sizeof(efes_extent), offsetof(efes_extent, length), sizeof(efes_objects), sizeof(efes_objects_out),
                EFES_OBJECTS_FRESH, EFES_OBJECTS_RUNNING, EFES_OBJECTS_MAX, EFES_OBJECTS_COPY_ALIGN%s};
  for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);
  return 0;
}""" % fields)
    exe = tmp_path / "objects"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    E, O, U = efes_lib.Extent, efes_lib.Objects, efes_lib.ObjectsOut
    assert got[:4] == [16, 8, 96, 32]
    assert got[:4] == [ctypes.sizeof(E), E.length.offset, ctypes.sizeof(O), ctypes.sizeof(U)]
    assert got[4:8] == [efes_lib.EFES_OBJECTS_FRESH, efes_lib.EFES_OBJECTS_RUNNING, efes_lib.EFES_OBJECTS_MAX,
                        efes_lib.EFES_OBJECTS_COPY_ALIGN] == [1, 2, 1 << 20, 256]
    assert got[8:] == [getattr(O, f).offset for f in OBJECT_FIELDS] + [getattr(U, f).offset for f in OUT_FIELDS]
    assert [f for f, _ in O._fields_] == OBJECT_FIELDS and [f for f, _ in U._fields_] == OUT_FIELDS
    assert efes_lib.EXTENT_DTYPE.itemsize == 16 and efes_lib.EXTENT_DTYPE.fields["length"][1] == 8


def _good(efes_lib, n=4, m=2):
    """A table and outputs that pass every check (host arrays; the device call fails only on its NULL context)."""
    keep = dict(ext=np.zeros((n, 2), np.uint64), first=np.array([0, 1, n][: m + 1], np.uint32), offs=np.zeros(m, np.uint64),
                jobs=np.zeros(n, efes_lib.JOB_DTYPE), dst=np.zeros(n, np.uint64), ck=np.zeros(n, np.uint64),
                lay=np.zeros(m + 1, np.uint64))
    t = efes_lib.Objects(data=0x1000, extents=keep["ext"].ctypes.data, first=keep["first"].ctypes.data, sha1=0x2000, crc32=0x3000,
                         sums=0x4000, status=0x5000, ckpt=0x6000, copy_to=0x7000, copy_offsets=keep["offs"].ctypes.data,
                         nobjects=m, nextents=n, flags=3, copy_align=64)
    o = efes_lib.ObjectsOut(jobs=keep["jobs"].ctypes.data, dst=keep["dst"].ctypes.data, ckpt=keep["ck"].ctypes.data,
                            layout=keep["lay"].ctypes.data)
    return t, o, keep


BAD = [("extents", None), ("first", None), ("sums", None), ("jobs", None), ("both_hashes", None), ("dst", None),
       ("out_ckpt", None), ("offsets_without_copy", None), ("flags", 4), ("flags", 0x80000000), ("copy_align", 3),
       ("copy_align", 96), ("copy_align", 1 << 21), ("nobjects", (1 << 20) + 1), ("nextents", (1 << 20) + 1)]


def _spoil(t, o, what, value):
    if what in ("extents", "first", "sums"):
        setattr(t, what, None)
    elif what == "jobs":
        o.jobs = None
    elif what == "both_hashes":
        t.sha1 = t.crc32 = None
    elif what == "dst":
        o.dst = None
    elif what == "out_ckpt":
        o.ckpt = None
    elif what == "offsets_without_copy":
        t.copy_to, o.dst = None, None
    else:
        setattr(t, what, value)


def test_the_good_table_passes(efes_lib):
    L = efes_lib.lib()
    t, o, keep = _good(efes_lib)
    assert L.efes_objects_jobs_host(ctypes.byref(t), ctypes.byref(o)) == efes_lib.EFES_OK
    for align in (0, 1, 2, 256, 1 << 20):
        t.copy_align = align
        assert L.efes_objects_jobs_host(ctypes.byref(t), ctypes.byref(o)) == efes_lib.EFES_OK, align
    # the largest counts are not refused for their size (no extents: nothing is read or written)
    big = efes_lib.Objects(nobjects=1 << 20, nextents=0)
    assert L.efes_objects_jobs_host(ctypes.byref(big), ctypes.byref(efes_lib.ObjectsOut())) == efes_lib.EFES_OK


@pytest.mark.parametrize("what,value", BAD)
def test_argument_errors_that_need_no_device(efes_lib, what, value):
    """By efes_objects_jobs_host, and by efes_objects_jobs in front of everything that needs its context: here with
    a NULL context, which is EFES_ERR_ARG on its own, so the device call is also given a good table below."""
    L = efes_lib.lib()
    t, o, keep = _good(efes_lib)
    _spoil(t, o, what, value)
    before = {k: v.copy() for k, v in keep.items()}
    assert L.efes_objects_jobs_host(ctypes.byref(t), ctypes.byref(o)) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_jobs(None, ctypes.byref(t), ctypes.byref(o), None, 0, None) == efes_lib.EFES_ERR_ARG
    assert all((keep[k] == before[k]).all() for k in keep), "a refused call wrote something"


def test_null_arguments(efes_lib):
    L = efes_lib.lib()
    t, o, keep = _good(efes_lib)
    assert L.efes_objects_jobs_host(None, ctypes.byref(o)) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_jobs_host(ctypes.byref(t), None) == efes_lib.EFES_ERR_ARG
    # a NULL context with a table that is fine otherwise, with and without extents
    assert L.efes_objects_jobs(None, ctypes.byref(t), ctypes.byref(o), None, 0, None) == efes_lib.EFES_ERR_ARG
    none = efes_lib.Objects()
    assert L.efes_objects_jobs(None, ctypes.byref(none), ctypes.byref(efes_lib.ObjectsOut()), None, 0, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_jobs(None, None, None, None, 0, None) == efes_lib.EFES_ERR_ARG


def test_with_no_extents_only_the_counts_are_checked(efes_lib):
    """The pointer, flag and alignment checks hold with nextents > 0; a table without extents passes them."""
    L = efes_lib.lib()
    t = efes_lib.Objects(nobjects=5, nextents=0, flags=0xFF, copy_align=3)
    assert L.efes_objects_jobs_host(ctypes.byref(t), ctypes.byref(efes_lib.ObjectsOut())) == efes_lib.EFES_OK
    t.nobjects = (1 << 20) + 1
    assert L.efes_objects_jobs_host(ctypes.byref(t), ctypes.byref(efes_lib.ObjectsOut())) == efes_lib.EFES_ERR_ARG


def test_scratch_size(efes_lib):
    from efes_amd.hashing import objects_jobs_scratch as scratch
    top = 1 << 20
    assert scratch(top + 1, 1) == 0 and scratch(1, top + 1) == 0 and scratch(top + 1, top + 1) == 0
    counts = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2051, 65536, top - 1, top]
    for m in counts:
        sizes = [scratch(m, n) for n in counts]
        assert sizes == sorted(sizes) and all(s % 16 == 0 for s in sizes), (m, sizes)
        assert all(s >= 8 * (n + 1) + 8 * (m + 1) for s, n in zip(sizes, counts)), m
    for n in counts:
        sizes = [scratch(m, n) for m in counts]
        assert sizes == sorted(sizes), (n, sizes)
    assert scratch(top, top) < 17 << 20  # 8 bytes per extent and per object, and the block sums


@pytest.mark.parametrize("build", ["Device", "gpu", "", None, 1])
def test_device_objects_rejects_unknown_builds(efes_lib, build):
    """Raised from the argument alone, before any context or device is touched."""
    from efes_amd.batch import DeviceObjects
    with pytest.raises(ValueError, match="build="):
        DeviceObjects(0x1000, [[(0, 16)]], build=build)
    with pytest.raises(ValueError, match="build="):
        DeviceObjects(0x1000, [[(0, 16)]], sha1=True, walk="wide", copy_to=0x100000, build=build)
