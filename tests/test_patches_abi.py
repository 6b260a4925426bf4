"""PATCH logs (efes_patches_table, efes_patches_table_scratch and the _host twin) without a GPU: the symbols and their
declarations, the struct layouts against the ctypes and numpy mirrors, the ABI version they leave alone, the build
lists, and every argument error -- by the twin, and by the device call in front of anything that needs its context."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")
NAMES = {"efes_patches_table_scratch": ("size_t", ["nobjects", "npatches"]),
         "efes_patches_table": ("int", ["ctx", "in", "scratch_device", "scratch_bytes", "stream"]),
         "efes_patches_table_host": ("int", ["in"])}
FIELDS = {"efes_patch": ["data_offset", "length", "file_offset", "file_length", "object", "_reserved"],
          "efes_patch_answer": ["offset", "verdict", "slot"],
          "efes_patch_object": ["offset", "flags", "admitted"],
          "efes_patches": ["log", "offsets", "sha1", "crc32", "extents", "first", "answers", "objects", "patch_of", "counts", "nobjects", "npatches"]}
SENTINEL = 0xA5
OUTPUTS = ("extents", "first", "answers", "objects", "patch_of", "counts", "sha1", "crc32")


def test_symbols_are_declared_and_exported(efes_lib):
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, (ret, want) in NAMES.items():
        m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (ret, name), header)
        assert m, f"{name} is not declared in efes_hash.h"
        args = [a.strip().split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
        assert args == want, (name, args)
        assert getattr(efes_lib.lib(), name)
        assert len(efes_lib.SIGNATURES[name][1]) == len(args)
    from efes_amd import hashing
    assert hasattr(hashing.Context, "patches_table") and hashing.patches_table_host and hashing.patches_table_scratch
    from efes_amd.batch import DeviceObjects
    assert DeviceObjects.from_patches and DeviceObjects.patch_answers_host and DeviceObjects.patch_objects_host
    assert DeviceObjects.patch_counts and DeviceObjects.patch_of_host
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "efes_patches_table" in open(os.path.join(ROOT, doc)).read(), doc


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8
    assert re.search(r"#define\s+EFES_ABI_VERSION\s+8\b", open(HEADER).read())


def test_build_id_covers_the_new_files(efes_lib):
    from efes_amd import build
    assert "efes_patches.hip" in build.SOURCES and "efes_patches.cpp" in build.SOURCES and "efes_patches_rules.hpp" in build.HEADERS
    assert efes_lib.lib().efes_build_id().decode() == build.source_id()


def test_struct_layouts_and_constants_match_header(tmp_path, efes_lib):
    prog = tmp_path / "patches.c"
    consts = ["EFES_PATCH_ADMITTED", "EFES_PATCH_CONFLICT", "EFES_PATCH_DEFERRED", "EFES_PATCH_DONE", "EFES_PATCH_INVALID",
              "EFES_PATCH_OBJ_RESTARTED", "EFES_PATCH_OBJ_DONE", "EFES_PATCH_OBJ_DEFERRED", "EFES_PATCH_LENGTH_UNKNOWN"]
    items = [f"sizeof({s})" for s in FIELDS] + [f"offsetof({s}, {f})" for s, fs in FIELDS.items() for f in fs] + consts
    prog.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "efes_hash.h"
int main(void) {
  unsigned long long v[] = {%s};
  for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf("%%llu ", v[i]);
  return 0;
}""" % ", ".join(f"(unsigned long long)({x})" for x in items))
    exe = tmp_path / "patches"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    E = efes_lib
    mirrors = {"efes_patch": E.Patch, "efes_patch_answer": E.PatchAnswer, "efes_patch_object": E.PatchObject, "efes_patches": E.Patches}
    assert got[:4] == [40, 16, 16, 88] == [ctypes.sizeof(mirrors[s]) for s in FIELDS]
    assert [E.PATCH_DTYPE.itemsize, E.PATCH_ANSWER_DTYPE.itemsize, E.PATCH_OBJECT_DTYPE.itemsize] == [40, 16, 16]
    at = 4
    for s, fs in FIELDS.items():
        assert [f for f, _ in mirrors[s]._fields_] == fs
        assert got[at:at + len(fs)] == [getattr(mirrors[s], f).offset for f in fs], s
        at += len(fs)
    for s, dt in (("efes_patch", E.PATCH_DTYPE), ("efes_patch_answer", E.PATCH_ANSWER_DTYPE), ("efes_patch_object", E.PATCH_OBJECT_DTYPE)):
        assert list(dt.names) == FIELDS[s] and [dt.fields[f][1] for f in dt.names] == [getattr(mirrors[s], f).offset for f in FIELDS[s]]
    assert got[at:] == [0, 1, 2, 3, 4, 1, 2, 4, (1 << 64) - 1]
    assert got[at:] == [E.EFES_PATCH_ADMITTED, E.EFES_PATCH_CONFLICT, E.EFES_PATCH_DEFERRED, E.EFES_PATCH_DONE, E.EFES_PATCH_INVALID,
                        E.EFES_PATCH_OBJ_RESTARTED, E.EFES_PATCH_OBJ_DONE, E.EFES_PATCH_OBJ_DEFERRED, E.EFES_PATCH_LENGTH_UNKNOWN]


def test_scratch_size(efes_lib):
    L = efes_lib.lib()
    top = efes_lib.EFES_OBJECTS_MAX
    assert L.efes_patches_table_scratch(0, 0) >= 16 and L.efes_patches_table_scratch(5, 0) >= 16
    assert L.efes_patches_table_scratch(top + 1, 1) == 0 and L.efes_patches_table_scratch(1, top + 1) == 0
    sizes = [L.efes_patches_table_scratch(m, n) for m, n in ((1, 1), (1, 1024), (1, 1025), (top, top))]
    assert all(s % 16 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] >= 16 * top
    assert L.efes_patches_table_scratch(1, 4096) == L.efes_patches_table_scratch(top, 4096), "the scratch depends on the PATCHes alone"


def _good(efes_lib, m=3, n=4):
    """A request that passes every check; the arrays (kept alive in `keep`) are sentinel-filled and lie 16 bytes into
    their buffers, so that a pointer may be moved off its alignment.  The log is four PATCHes at offset 0."""
    log = np.zeros(n, efes_lib.PATCH_DTYPE)
    log["object"], log["length"] = np.arange(n) % m, 5
    sizes = dict(extents=16 * n, first=4 * (m + 1), answers=16 * n, objects=16 * m, patch_of=4 * n, counts=20, sha1=104 * m, crc32=4 * m)
    keep = {k: np.full(size + 32, SENTINEL, np.uint8) for k, size in sizes.items()}
    keep["log"] = np.concatenate((np.zeros(16, np.uint8), log.view(np.uint8), np.zeros(16, np.uint8)))
    keep["offsets"] = np.zeros(8 * m + 32, np.uint8)
    keep["scratch"] = np.zeros(1 << 16, np.uint8)
    at = lambda k: keep[k].ctypes.data + 16
    assert all(at(k) % 8 == 0 for k in keep)
    return efes_lib.Patches(nobjects=m, npatches=n, **{k: at(k) for k in keep if k != "scratch"}), keep


def _untouched(keep):
    return all((keep[k] == SENTINEL).all() for k in OUTPUTS)


def _scratch(keep):
    return keep["scratch"].ctypes.data + (-keep["scratch"].ctypes.data) % 16


# (field, value): None = the pointer NULLed, an int for a pointer = moved off its alignment by that many bytes
BAD = [("nobjects", (1 << 20) + 1), ("nobjects", 0xFFFFFFFF), ("npatches", (1 << 20) + 1), ("npatches", 0xFFFFFFFF), ("nobjects", 0),
       ("log", None), ("extents", None), ("first", None),
       ("log", +4), ("log", +1), ("offsets", +4), ("offsets", +2), ("sha1", +4), ("sha1", +1), ("extents", +4), ("extents", +2),
       ("answers", +4), ("answers", +1), ("objects", +4), ("objects", +2),
       ("crc32", +2), ("crc32", +1), ("first", +2), ("first", +1), ("patch_of", +2), ("patch_of", +3), ("counts", +2), ("counts", +1)]


def _spoil(r, what, value):
    if value is None or what in ("nobjects", "npatches"):
        setattr(r, what, value)
    else:
        setattr(r, what, getattr(r, what) + value)


def test_the_good_request_passes(efes_lib):
    L = efes_lib.lib()
    r, keep = _good(efes_lib)
    assert L.efes_patches_table_host(ctypes.byref(r)) == efes_lib.EFES_OK
    assert keep["first"][16:32].view(np.uint32).tolist() == [0, 2, 3, 4]
    assert keep["counts"][16:36].view(np.uint32).tolist() == [3, 0, 1, 0, 0], "object 0's second PATCH at offset 0 is deferred"
    assert all((keep[k][:16] == SENTINEL).all() and (keep[k][-16:] == SENTINEL).all() for k in OUTPUTS)
    for drop in ("offsets", "sha1", "crc32", "answers", "objects", "patch_of", "counts"):  # each may be NULL
        r2, _ = _good(efes_lib)
        setattr(r2, drop, None)
        assert L.efes_patches_table_host(ctypes.byref(r2)) == efes_lib.EFES_OK
    # 4-byte alignment is enough for the arrays of words
    for what in ("crc32", "first", "patch_of", "counts"):
        r2, _ = _good(efes_lib)
        _spoil(r2, what, 4)
        assert L.efes_patches_table_host(ctypes.byref(r2)) == efes_lib.EFES_OK
    # npatches == 0: first (all zeros), objects and counts are written, and nothing else; log and extents may be NULL
    r, keep = _good(efes_lib)
    r.npatches, r.log, r.extents = 0, None, None
    assert L.efes_patches_table_host(ctypes.byref(r)) == efes_lib.EFES_OK
    assert keep["first"][16:32].view(np.uint32).tolist() == [0] * 4 and keep["counts"][16:36].view(np.uint32).tolist() == [0] * 5
    assert keep["objects"][16:64].view(efes_lib.PATCH_OBJECT_DTYPE).tolist() == [(0, 0, 0)] * 3
    assert all((keep[k] == SENTINEL).all() for k in ("extents", "answers", "patch_of", "sha1", "crc32"))
    # no objects and no PATCHes: first[0] alone
    r.nobjects = 0
    assert L.efes_patches_table_host(ctypes.byref(r)) == efes_lib.EFES_OK


@pytest.mark.parametrize("what,value", BAD)
def test_argument_errors_that_need_no_device(efes_lib, what, value):
    """By the twin, and by the device call in front of everything that needs its context (here with a NULL context,
    which is EFES_ERR_ARG on its own).  A refused call leaves the sentinel-filled outputs alone."""
    L = efes_lib.lib()
    r, keep = _good(efes_lib)
    _spoil(r, what, value)
    assert L.efes_patches_table_host(ctypes.byref(r)) == efes_lib.EFES_ERR_ARG
    assert L.efes_patches_table(None, ctypes.byref(r), _scratch(keep), 1 << 15, None) == efes_lib.EFES_ERR_ARG
    assert _untouched(keep), "a refused call wrote something"


def test_null_arguments_and_scratch(efes_lib):
    L = efes_lib.lib()
    r, keep = _good(efes_lib)
    assert L.efes_patches_table_host(None) == efes_lib.EFES_ERR_ARG
    assert L.efes_patches_table(None, None, _scratch(keep), 1 << 15, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_patches_table(None, ctypes.byref(r), _scratch(keep), 1 << 15, None) == efes_lib.EFES_ERR_ARG  # a NULL context alone
    for scratch, size in ((None, 1 << 15), (_scratch(keep) + 8, 1 << 15), (_scratch(keep), L.efes_patches_table_scratch(3, 4) - 1), (_scratch(keep), 0)):
        assert L.efes_patches_table(None, ctypes.byref(r), scratch, size, None) == efes_lib.EFES_ERR_ARG
    assert _untouched(keep)


def test_from_patches_checks_its_arguments_before_any_device(efes_lib):
    """From the arguments alone, before a context, a device or a tensor is touched (this machine has none)."""
    from efes_amd.batch import DeviceObjects
    log = np.zeros(3, efes_lib.PATCH_DTYPE)
    with pytest.raises(ValueError, match="PATCH_DTYPE"):
        DeviceObjects.from_patches(0x1000, np.zeros(120, np.uint8), nobjects=2)
    with pytest.raises(ValueError, match="nobjects="):
        DeviceObjects.from_patches(0x1000, log)
    with pytest.raises(ValueError, match="offsets has not 2"):
        DeviceObjects.from_patches(0x1000, log, np.zeros(3, np.uint64), nobjects=2)
    for walk in ("auto", "auto_wide"):
        with pytest.raises(ValueError, match="chain count"):
            DeviceObjects.from_patches(0x1000, log, nobjects=2, sha1=True, walk=walk)
    with pytest.raises(ValueError, match="walk="):
        DeviceObjects.from_patches(0x1000, log, nobjects=2, walk="wide")
    with pytest.raises(ValueError, match="infos="):
        DeviceObjects.from_patches(0x1000, log, nobjects=2, sha1=True, infos=np.full((2, 208), ord("0"), np.uint8), crcs=np.zeros(2, np.uint32))
    O = DeviceObjects.__new__(DeviceObjects)
    for call in (O.patch_answers_host, O.patch_objects_host, O.patch_counts, O.patch_of_host):
        with pytest.raises(ValueError, match="from_patches"):
            call()
