"""Object infos (efes_infos_unmarshal_text, efes_infos_marshal_text and their _host twins) without a GPU: the symbols
and their declarations, the struct layout against the ctypes mirror, the ABI version they leave alone, every argument
error (by the twins, and by the device calls in front of anything that needs their context), and the argument checks
of DeviceObjects(infos=)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")
NAMES = {"efes_infos_unmarshal_text": ["ctx", "in", "stream"], "efes_infos_marshal_text": ["ctx", "in", "stream"],
         "efes_infos_unmarshal_text_host": ["in"], "efes_infos_marshal_text_host": ["in"]}
FIELDS = ["text", "sha1", "crc32", "status", "counts", "n", "_reserved"]
SENTINEL = 0xA5
OUTPUTS = ("text", "sha1", "crc32", "status", "counts")


def test_symbols_are_declared_and_exported(efes_lib):
    header = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name, want in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m, f"{name} is not declared in efes_hash.h"
        args = [a.strip().split()[-1].lstrip("*") for a in " ".join(m.group(1).split()).split(",")]
        assert args == want, (name, args)
        assert getattr(efes_lib.lib(), name)
        assert len(efes_lib.SIGNATURES[name][1]) == len(args)
    from efes_amd import hashing
    assert hasattr(hashing.Context, "infos_unmarshal_text") and hasattr(hashing.Context, "infos_marshal_text")
    assert hashing.infos_unmarshal_text_host and hashing.infos_marshal_text_host
    from efes_amd.batch import DeviceObjects
    assert DeviceObjects.info_texts and DeviceObjects.resume_counts and DeviceObjects.resume_status_host
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "efes_infos_unmarshal_text" in open(os.path.join(ROOT, doc)).read(), doc


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8
    assert re.search(r"#define\s+EFES_ABI_VERSION\s+8\b", open(HEADER).read())


def test_build_id_covers_the_new_files(efes_lib):
    from efes_amd import build
    assert "efes_infos.hip" in build.SOURCES and "efes_infos.cpp" in build.SOURCES and "efes_infos_rules.hpp" in build.HEADERS
    assert efes_lib.lib().efes_build_id().decode() == build.source_id()


def test_struct_layout_and_constants_match_header(tmp_path, efes_lib):
    prog = tmp_path / "infos.c"
    prog.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "efes_hash.h"
int main(void) {
  size_t v[] = {sizeof(efes_infos), EFES_INFO_TEXT_BYTES, EFES_SHA1_NX_REFUSED, EFES_CHECKPOINT_TEXT_BYTES%s};
  for (size_t i = 0; i < sizeof v / sizeof *v; ++i) printf("%%zu ", v[i]);
  return 0;
}""" % "".join(f", offsetof(efes_infos, {f})" for f in FIELDS))
    exe = tmp_path / "infos"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    I = efes_lib.Infos
    assert got[0] == 48 == ctypes.sizeof(I)
    assert got[1:4] == [208, 65, 208] == [efes_lib.EFES_INFO_TEXT_BYTES, efes_lib.EFES_SHA1_NX_REFUSED, efes_lib.CHECKPOINT_TEXT_BYTES]
    assert got[4:] == [getattr(I, f).offset for f in FIELDS] and [f for f, _ in I._fields_] == FIELDS


def _good(efes_lib, n=3):
    """A request that passes every check; the arrays (kept alive in `keep`) are sentinel-filled and lie 16 bytes into
    their buffers, so that a pointer may be moved off its alignment.  The texts are all '0': valid."""
    keep = dict(text=np.full(208 * n + 32, ord("0"), np.uint8), sha1=np.full(104 * n + 32, SENTINEL, np.uint8),
                crc32=np.full(4 * n + 32, SENTINEL, np.uint8), status=np.full(4 * n + 32, SENTINEL, np.uint8),
                counts=np.full(8 + 32, SENTINEL, np.uint8))
    at = lambda k: keep[k].ctypes.data + 16
    assert all(at(k) % 8 == 0 for k in keep)
    return efes_lib.Infos(text=at("text"), sha1=at("sha1"), crc32=at("crc32"), status=at("status"), counts=at("counts"), n=n), keep


def _untouched(keep, text_too=True):
    return all((keep[k] == (ord("0") if k == "text" else SENTINEL)).all() for k in OUTPUTS if text_too or k != "text")


# (field, value): None = the pointer NULLed, an int for a pointer = moved off its alignment by that many bytes
BAD_BOTH = [("n", (1 << 20) + 1), ("n", 0xFFFFFFFF), ("_reserved", 1), ("_reserved", 0x80000000), ("text", None), ("both", None),
            ("sha1", +4), ("sha1", +1), ("sha1", +2), ("crc32", +2), ("crc32", +1), ("status", +2), ("status", +3),
            ("counts", +2), ("counts", +1)]
BAD_DEVICE_ONLY = [("text", +4), ("text", +1), ("text", +2)]


def _spoil(r, what, value):
    if what == "both":
        r.sha1 = r.crc32 = None
    elif value is None or what in ("n", "_reserved"):
        setattr(r, what, value)
    else:
        setattr(r, what, getattr(r, what) + value)


def test_the_good_request_passes(efes_lib):
    L = efes_lib.lib()
    r, keep = _good(efes_lib)
    assert L.efes_infos_unmarshal_text_host(ctypes.byref(r)) == efes_lib.EFES_OK
    assert keep["counts"][16:24].view(np.uint32).tolist() == [3, 0]
    assert (keep["sha1"][16:16 + 312] == 0).all() and (keep["crc32"][16:28] == 0).all() and (keep["status"][16:28] == 0).all()
    assert all((keep[k][:16] == SENTINEL).all() and (keep[k][-16:] == SENTINEL).all() for k in OUTPUTS if k != "text")
    assert L.efes_infos_marshal_text_host(ctypes.byref(r)) == efes_lib.EFES_OK
    assert (keep["text"] == ord("0")).all()
    for drop in ("sha1", "crc32", "status", "counts"):  # each may be NULL (sha1 and crc32 not both)
        r2, _ = _good(efes_lib)
        setattr(r2, drop, None)
        assert L.efes_infos_unmarshal_text_host(ctypes.byref(r2)) == efes_lib.EFES_OK
        assert L.efes_infos_marshal_text_host(ctypes.byref(r2)) == efes_lib.EFES_OK
    # the largest count is not refused for its size; nothing to do: every pointer may be NULL
    none = efes_lib.Infos()
    assert L.efes_infos_unmarshal_text_host(ctypes.byref(none)) == efes_lib.EFES_OK
    assert L.efes_infos_marshal_text_host(ctypes.byref(none)) == efes_lib.EFES_OK
    # n == 0 still writes counts, whole, and nothing else
    r, keep = _good(efes_lib)
    r.n = 0
    assert L.efes_infos_unmarshal_text_host(ctypes.byref(r)) == efes_lib.EFES_OK
    assert keep["counts"][16:24].view(np.uint32).tolist() == [0, 0] and (keep["counts"][24:] == SENTINEL).all()
    assert all((keep[k] == SENTINEL).all() for k in ("sha1", "crc32", "status"))
    # the twins take text at any alignment
    for off in (1, 2, 3, 4, 5, 7):
        r, keep = _good(efes_lib)
        r.text += off
        assert L.efes_infos_unmarshal_text_host(ctypes.byref(r)) == efes_lib.EFES_OK
        assert L.efes_infos_marshal_text_host(ctypes.byref(r)) == efes_lib.EFES_OK


@pytest.mark.parametrize("what,value", BAD_BOTH)
def test_argument_errors_that_need_no_device(efes_lib, what, value):
    """By the twins, and by the device calls in front of everything that needs their context (here with a NULL
    context, which is EFES_ERR_ARG on its own).  A refused call leaves the sentinel-filled outputs alone."""
    L = efes_lib.lib()
    r, keep = _good(efes_lib)
    _spoil(r, what, value)
    for call in (L.efes_infos_unmarshal_text_host, L.efes_infos_marshal_text_host):
        assert call(ctypes.byref(r)) == efes_lib.EFES_ERR_ARG
    for call in (L.efes_infos_unmarshal_text, L.efes_infos_marshal_text):
        assert call(None, ctypes.byref(r), None) == efes_lib.EFES_ERR_ARG
    assert _untouched(keep), "a refused call wrote something"


@pytest.mark.parametrize("what,value", BAD_DEVICE_ONLY)
def test_text_alignment_is_the_device_calls_alone(efes_lib, what, value):
    L = efes_lib.lib()
    r, keep = _good(efes_lib)
    _spoil(r, what, value)
    for call in (L.efes_infos_unmarshal_text, L.efes_infos_marshal_text):
        assert call(None, ctypes.byref(r), None) == efes_lib.EFES_ERR_ARG
    assert _untouched(keep)
    assert L.efes_infos_unmarshal_text_host(ctypes.byref(r)) == efes_lib.EFES_OK


def test_null_arguments(efes_lib):
    L = efes_lib.lib()
    r, keep = _good(efes_lib)
    assert L.efes_infos_unmarshal_text_host(None) == efes_lib.EFES_ERR_ARG
    assert L.efes_infos_marshal_text_host(None) == efes_lib.EFES_ERR_ARG
    for call in (L.efes_infos_unmarshal_text, L.efes_infos_marshal_text):
        assert call(None, None, None) == efes_lib.EFES_ERR_ARG
        assert call(None, ctypes.byref(r), None) == efes_lib.EFES_ERR_ARG  # a NULL context with a good request
    assert _untouched(keep)
    # the pointer checks depend on n: text and one of the states only with records
    r.n, r.text, r.sha1, r.crc32 = 0, None, None, None
    assert L.efes_infos_unmarshal_text_host(ctypes.byref(r)) == efes_lib.EFES_OK
    r.n = 1
    assert L.efes_infos_unmarshal_text_host(ctypes.byref(r)) == efes_lib.EFES_ERR_ARG


def test_device_objects_checks_infos_before_any_device(efes_lib):
    """infos= with fresh=True, states= or crcs= raises, and so do wrong shapes: from the arguments alone, before a
    context, a device or a tensor is touched (this machine has none)."""
    from efes_amd.batch import DeviceObjects, fresh_states
    objects = [[(0, 10)], [(10, 5), (20, 5)], []]
    good = np.full((3, 208), ord("0"), np.uint8)
    pairs = [(b"0" * 200, b"0" * 8)] * 3
    for kw in (dict(fresh=True), dict(states=fresh_states(3)), dict(crcs=np.zeros(3, np.uint32)),
               dict(states=fresh_states(3), crcs=np.zeros(3, np.uint32))):
        for infos in (good, pairs):
            with pytest.raises(ValueError, match="infos="):
                DeviceObjects(0x1000, objects, sha1=True, infos=infos, **kw)
    for infos in (good[:2], good[:, :200], good.reshape(-1), good.astype(np.uint32), np.zeros((3, 208, 1), np.uint8), pairs[:2],
                  pairs + pairs[:1], [b"0" * 208] * 3, [(b"0" * 200,)] * 3):
        with pytest.raises(ValueError, match="infos is 3 x 208"):
            DeviceObjects(0x1000, objects, sha1=True, infos=infos)
        with pytest.raises(ValueError, match="infos is 3 x 208"):
            DeviceObjects(0x1000, objects, sha1=True, infos=infos, build="device")
    # what the checks hand on: infos implies fresh=False; a pair of the wrong length becomes a row of b"?"
    fresh, rows = DeviceObjects._check_infos([(b"a" * 200, b"b" * 8), (b"a" * 199, b"b" * 8), ("c" * 200, "d" * 7)], None, None, None, 3)
    assert fresh is False and rows.shape == (3, 208) and rows.dtype == np.uint8
    assert bytes(rows[0]) == b"a" * 200 + b"b" * 8 and bytes(rows[1]) == b"?" * 208 == bytes(rows[2])
    assert DeviceObjects._check_infos(None, None, None, None, 3) == (True, None)
    assert DeviceObjects._check_infos(None, False, None, None, 3) == (False, None)
    assert DeviceObjects._check_infos(good, False, None, None, 3)[0] is False
    # the accessors of a set that was not resumed from texts say so
    O = DeviceObjects.__new__(DeviceObjects)
    for call in (O.resume_counts, O.resume_status_host):
        with pytest.raises(ValueError, match="infos="):
            call()
