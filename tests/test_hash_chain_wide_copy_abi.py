"""The wide chain walk with copy (efes_hash_chain_wide_copy) without a GPU: the symbol and its declaration, the
ABI version it leaves alone, the argument errors that need no device, and the argument checks of
DeviceObjects(sha1=True, copy_to=...), which gathers only through walk="wide"."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")


def test_symbol_is_declared_and_exported(efes_lib):
    header = open(HEADER).read()
    m = re.search(r"\bint\s+efes_hash_chain_wide_copy\s*\(([^;]*)\)\s*;", header)
    assert m, "efes_hash_chain_wide_copy is not declared in efes_hash.h"
    args = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["ctx", "jobs_device", "dst_device", "ckpt_device", "njobs",
                                                         "scratch_device", "scratch_bytes", "stream"], args
    assert efes_lib.lib().efes_hash_chain_wide_copy
    assert "efes_hash_chain_wide_copy" in efes_lib.SIGNATURES
    assert len(efes_lib.SIGNATURES["efes_hash_chain_wide_copy"][1]) == len(args)
    from efes_amd import hashing
    assert hasattr(hashing.Context, "hash_chain_wide_copy")


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8
    assert re.search(r"#define\s+EFES_ABI_VERSION\s+8\b", open(HEADER).read())


def test_argument_errors_that_need_no_device(efes_lib):
    L = efes_lib.lib()
    job = efes_lib.Job()
    dst = (ctypes.c_void_p * 1)(None)
    j, d = ctypes.addressof(job), ctypes.addressof(dst)
    f = L.efes_hash_chain_wide_copy
    # a NULL context, with and without jobs
    assert f(None, None, None, None, 0, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert f(None, j, d, None, 1, None, 0, None) == efes_lib.EFES_ERR_ARG
    # NULL jobs and a NULL dst_device with njobs > 0 are refused before the context is looked at any further
    assert f(None, None, d, None, 1, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert f(None, j, None, None, 1, None, 0, None) == efes_lib.EFES_ERR_ARG


@pytest.mark.parametrize("walk", [None, "auto", "auto_wide", "GROUP16"])
@pytest.mark.parametrize("crc32", [True, False])
def test_device_objects_copy_needs_the_wide_walk(efes_lib, walk, crc32):
    """Raised from the arguments alone, before any context or device is touched; the message names walk="wide"."""
    from efes_amd.batch import DeviceObjects
    w = efes_lib.MODE_GROUP[16] if walk == "GROUP16" else walk
    with pytest.raises(ValueError, match='walk="wide"'):
        DeviceObjects(0x1000, [[(0, 16)]], sha1=True, crc32=crc32, walk=w, copy_to=0x100000)
    with pytest.raises(ValueError, match='walk="wide"'):
        DeviceObjects(0x1000, [[(0, 16)]], sha1=True, crc32=crc32, walk=w, copy_to=0x100000, checkpoints=True)


def test_device_objects_wide_copy_passes_the_argument_checks(efes_lib):
    """walk="wide" with copy_to= is past every ValueError of the argument checks: without a device the
    constructor ends in the context's error (an EfesError or torch's), with one it builds the set.  The
    copy_offsets= without copy_to= error stays, and so does the CRC-only set's refusal of walk=."""
    from efes_amd.batch import DeviceObjects
    for kw in (dict(), dict(crc32=False), dict(checkpoints=True), dict(copy_offsets=[512])):
        try:
            O = DeviceObjects(0x1000, [[(0, 16), (64, 3)]], sha1=True, walk="wide", copy_to=0x100000, **kw)
        except ValueError as e:
            pytest.fail(f"{kw}: {e}")
        except Exception:
            continue  # no device: the argument checks are behind us
        assert O.wide and O.copy_to == 0x100000 and O.copy_bytes == (19 if "copy_offsets" not in kw else 512 + 19)
    with pytest.raises(ValueError, match="copy_offsets"):
        DeviceObjects(0x1000, [[(0, 16)]], sha1=True, walk="wide", copy_offsets=[0])
    with pytest.raises(ValueError):
        DeviceObjects(0x1000, [[(0, 16)]], walk="wide", copy_to=0x100000)
