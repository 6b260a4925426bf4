"""Object results (efes_objects_results, efes_objects_results_scratch, efes_objects_results_host) without a GPU: the
symbols and their declarations, the struct layouts against the ctypes mirrors, the ABI version they leave alone,
the verdict constants, every argument error that needs no device, the scratch size, and the argument checks of
DeviceObjects.verify()."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")
NAMES = {"efes_objects_results_scratch": ["nobjects", "nextents"],
         "efes_objects_results": ["ctx", "in", "req", "scratch_device", "scratch_bytes", "stream"],
         "efes_objects_results_host": ["in", "req"]}
RESULT_FIELDS = ["sum", "status", "verdict"]
REQUEST_FIELDS = ["expected", "compare", "_reserved", "results", "bad", "counts"]
SENTINEL = 0xA5


def test_symbols_are_declared_and_exported(efes_lib):
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want in NAMES.items():
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in efes_hash.h"
        args = [a.strip().split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
        assert args == want, (name, args)
        assert getattr(efes_lib.lib(), name)
        assert len(efes_lib.SIGNATURES[name][1]) == len(args)
    from efes_amd import hashing
    assert hasattr(hashing.Context, "objects_results") and hashing.objects_results_scratch and hashing.objects_results_host
    from efes_amd.batch import DeviceObjects
    assert DeviceObjects.verify and DeviceObjects.results


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8
    assert re.search(r"#define\s+EFES_ABI_VERSION\s+8\b", open(HEADER).read())


def test_struct_layouts_and_verdicts_match_header(tmp_path, efes_lib):
    prog = tmp_path / "results.c"
    fields = ("".join(f", offsetof(efes_object_result, {f})" for f in RESULT_FIELDS) +
              "".join(f", offsetof(efes_results, {f})" for f in REQUEST_FIELDS))
    prog.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "efes_hash.h"
int main(void) {
  size_t v[] = {sizeof(efes_object_result), sizeof(efes_results), EFES_VERDICT_OK, EFES_VERDICT_MISMATCH,
                EFES_VERDICT_FAILED, EFES_VERDICT_EMPTY, EFES_HASH_SHA1, EFES_HASH_CRC32%s};
  for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);
  return 0;
}""" % fields)
    exe = tmp_path / "results"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    O, R = efes_lib.ObjectResult, efes_lib.Results
    assert got[:2] == [32, 40] == [ctypes.sizeof(O), ctypes.sizeof(R)]
    assert got[2:6] == [0, 1, 2, 3] == [efes_lib.EFES_VERDICT_OK, efes_lib.EFES_VERDICT_MISMATCH, efes_lib.EFES_VERDICT_FAILED,
                                        efes_lib.EFES_VERDICT_EMPTY]
    assert got[6:8] == [efes_lib.EFES_HASH_SHA1, efes_lib.EFES_HASH_CRC32] == [1, 2]
    assert got[8:] == [getattr(O, f).offset for f in RESULT_FIELDS] + [getattr(R, f).offset for f in REQUEST_FIELDS]
    assert [f for f, _ in O._fields_] == RESULT_FIELDS and [f for f, _ in R._fields_] == REQUEST_FIELDS
    D = efes_lib.OBJECT_RESULT_DTYPE
    assert D.itemsize == 32 and [D.fields[f][1] for f in RESULT_FIELDS] == [0, 24, 28]


def _good(efes_lib, n=4, m=2):
    """A table and a request that pass every check; the arrays (kept alive in `keep`) are sentinel-filled outputs and
    inputs that lie 16 bytes into their buffers, so that a pointer may be moved off its alignment."""
    keep = dict(first=np.array([0, 1, n][: m + 1], np.uint32), status=np.zeros(n + 8, np.int32), sums=np.zeros(24 * n + 32, np.uint8),
                expected=np.zeros(24 * m + 32, np.uint8), results=np.full(32 * m + 32, SENTINEL, np.uint8),
                bad=np.full(4 * m + 32, SENTINEL, np.uint8), counts=np.full(16 + 32, SENTINEL, np.uint8))
    at = lambda k: keep[k].ctypes.data + 16
    t = efes_lib.Objects(first=keep["first"].ctypes.data, sums=at("sums"), status=at("status"), nobjects=m, nextents=n)
    r = efes_lib.Results(expected=at("expected"), compare=3, results=at("results"), bad=at("bad"), counts=at("counts"))
    return t, r, keep


BAD = [("counts", None), ("nobjects", (1 << 20) + 1), ("nextents", (1 << 20) + 1), ("compare", 4), ("compare", 0x80000001),
       ("_reserved", 1), ("first", None), ("sums", None), ("status", None), ("sums", +2), ("sums", +1), ("expected", +2),
       ("expected", +3), ("results", +4), ("results", +2), ("bad", +2), ("bad", +1), ("counts", +2), ("counts", +3)]


def _spoil(t, r, what, value):
    where = t if what in ("nobjects", "nextents", "first", "sums", "status") else r
    if value is None or what in ("nobjects", "nextents", "compare", "_reserved"):
        setattr(where, what, value)
    else:  # a pointer moved off its alignment
        setattr(where, what, getattr(where, what) + value)


def test_the_good_request_passes(efes_lib):
    L = efes_lib.lib()
    t, r, keep = _good(efes_lib)
    assert L.efes_objects_results_host(ctypes.byref(t), ctypes.byref(r)) == efes_lib.EFES_OK
    assert keep["counts"][16:32].view(np.uint32).tolist() == [2, 0, 0, 0]  # every status EFES_OK, the sums as expected
    for compare in (0, 1, 2, 3):
        r.compare = compare
        assert L.efes_objects_results_host(ctypes.byref(t), ctypes.byref(r)) == efes_lib.EFES_OK
    r.expected = r.results = r.bad = None  # each may be NULL
    assert L.efes_objects_results_host(ctypes.byref(t), ctypes.byref(r)) == efes_lib.EFES_OK
    # the largest counts are not refused for their size: no objects, nothing but the counters is written
    big = efes_lib.Objects(nobjects=0, nextents=1 << 20, sums=0x1000, status=0x1000)
    assert L.efes_objects_results_host(ctypes.byref(big), ctypes.byref(r)) == efes_lib.EFES_OK
    assert keep["counts"][16:32].view(np.uint32).tolist() == [0, 0, 0, 0]
    none = efes_lib.Objects()  # no objects, no extents: every table pointer may be NULL
    assert L.efes_objects_results_host(ctypes.byref(none), ctypes.byref(r)) == efes_lib.EFES_OK


@pytest.mark.parametrize("what,value", BAD)
def test_argument_errors_that_need_no_device(efes_lib, what, value):
    """By efes_objects_results_host, and by efes_objects_results in front of everything that needs its context (here
    with a NULL context, which is EFES_ERR_ARG on its own).  A refused call leaves the sentinel-filled outputs alone."""
    L = efes_lib.lib()
    t, r, keep = _good(efes_lib)
    _spoil(t, r, what, value)
    assert L.efes_objects_results_host(ctypes.byref(t), ctypes.byref(r)) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_results(None, ctypes.byref(t), ctypes.byref(r), None, 0, None) == efes_lib.EFES_ERR_ARG
    assert all((keep[k] == SENTINEL).all() for k in ("results", "bad", "counts")), "a refused call wrote something"


def test_null_arguments(efes_lib):
    L = efes_lib.lib()
    t, r, keep = _good(efes_lib)
    assert L.efes_objects_results_host(None, ctypes.byref(r)) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_results_host(ctypes.byref(t), None) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_results(None, ctypes.byref(t), ctypes.byref(r), None, 0, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_objects_results(None, None, None, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert all((keep[k] == SENTINEL).all() for k in ("results", "bad", "counts"))
    # the pointer checks depend on the counts: first with objects, sums and status with extents
    t.nobjects, t.nextents, t.first, t.sums, t.status = 0, 0, None, None, None
    assert L.efes_objects_results_host(ctypes.byref(t), ctypes.byref(r)) == efes_lib.EFES_OK
    t.nobjects = 1
    assert L.efes_objects_results_host(ctypes.byref(t), ctypes.byref(r)) == efes_lib.EFES_ERR_ARG


def test_scratch_size(efes_lib):
    from efes_amd.hashing import objects_results_scratch as scratch
    top = 1 << 20
    assert scratch(top + 1, 1) == 0 and scratch(1, top + 1) == 0 and scratch(top + 1, top + 1) == 0
    counts = [0, 1, 2, 63, 64, 65, 1023, 1024, 1025, 2051, 65536, top - 1, top]
    for m in counts:
        sizes = [scratch(m, n) for n in counts]
        assert sizes == sorted(sizes) and all(s and s % 16 == 0 for s in sizes), (m, sizes)
        assert all(s >= 4 * m for s in sizes), m  # a word per object for the first failing member
    for n in counts:
        sizes = [scratch(m, n) for m in counts]
        assert sizes == sorted(sizes), (n, sizes)
    assert scratch(top, top) < 16 << 20


def test_verify_checks_its_arguments_before_any_device(efes_lib):
    from efes_amd.batch import DeviceObjects
    O = DeviceObjects.__new__(DeviceObjects)  # no constructor: no context, no device, no tensor
    O.nobjects, O.n, O.has_sha1, O.has_crc32 = 5, 9, True, False
    good = np.zeros((5, 24), np.uint8)
    for expected in (np.zeros((4, 24), np.uint8), np.zeros((5, 20), np.uint8), np.zeros(120, np.uint8), np.zeros((5, 24), np.uint32),
                     np.zeros((5, 24, 1), np.uint8)):
        with pytest.raises(ValueError, match="expected"):
            O.verify(expected)
        with pytest.raises(ValueError, match="expected"):
            O.results(expected)
    for compare in (4, 7, -1, 1 << 31, "sha1", 1.0, True):
        with pytest.raises(ValueError, match="compare="):
            O.verify(good, compare)
        with pytest.raises(ValueError, match="compare="):
            O.results(compare=compare)
    # the default mask is the digests the set keeps
    assert O._results_args(good, None)[1] == efes_lib.EFES_HASH_SHA1
    O.has_crc32 = True
    assert O._results_args(good, None)[1] == efes_lib.EFES_HASH_SHA1 | efes_lib.EFES_HASH_CRC32
    assert O._results_args(None, 0) == (None, 0)
