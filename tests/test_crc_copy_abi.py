"""Copy with CRC (efes_crc32_copy) without a GPU: the scratch size, the argument errors that need no
device, the ABI version, which the purely additive call leaves at 8, and the host side of
DeviceObjects(copy_to=...): the refusal of SHA-1 sets and the default destination layout."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")
COUNTS = (1, 2, 1023, 1024, 1025, 65537)


def _header_constant(name: str) -> int:
    m = re.search(r"#define\s+%s\s+(\w+)" % name, open(HEADER).read())
    assert m, name
    return int(re.sub(r"u$", "", m.group(1)), 0)


def test_scratch_size(efes_lib):
    f, chain = efes_lib.lib().efes_crc32_copy_scratch, efes_lib.lib().efes_crc32_chain_scratch
    MAX = efes_lib.EFES_CRC_BATCH_MAX_JOBS
    assert f(0) == 0 and f(MAX + 1) == 0 and f(0xFFFFFFFF) == 0
    counts = COUNTS + (MAX,)
    sizes = [f(n) for n in counts]
    assert all(s > 0 for s in sizes), sizes
    assert sizes == sorted(sizes), sizes
    assert all(s >= chain(n) for s, n in zip(sizes, counts)), sizes


def test_python_wrappers_return_the_same_sizes(efes_lib):
    from efes_amd import hashing
    assert "crc32_copy_scratch" in hashing.__all__ and hasattr(hashing.Context, "crc32_copy")
    f = efes_lib.lib().efes_crc32_copy_scratch
    for n in (0,) + COUNTS + (efes_lib.EFES_CRC_BATCH_MAX_JOBS, efes_lib.EFES_CRC_BATCH_MAX_JOBS + 1):
        assert hashing.crc32_copy_scratch(n) == f(n), n
        assert hashing.crc32_copy_scratch(n) >= hashing.crc32_chain_scratch(n), n


def test_argument_errors_that_need_no_device(efes_lib):
    L = efes_lib.lib()
    job, dst = efes_lib.Job(), ctypes.c_void_p(0)
    # a NULL context
    assert L.efes_crc32_copy(None, None, None, 0, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_crc32_copy(None, ctypes.addressof(job), ctypes.addressof(dst), 1, None, 0, None) == efes_lib.EFES_ERR_ARG
    # a NULL dst_device with one job
    assert L.efes_crc32_copy(None, ctypes.addressof(job), None, 1, None, 0, None) == efes_lib.EFES_ERR_ARG


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8 == _header_constant("EFES_ABI_VERSION")
    assert "efes_crc32_copy" in open(HEADER).read()


def test_device_objects_copy_is_crc_only():
    """Raised from the arguments alone: no context, no device."""
    from efes_amd.batch import DeviceObjects
    with pytest.raises(ValueError):
        DeviceObjects(0x1000, [[(0, 16)]], sha1=True, copy_to=0x100000)
    with pytest.raises(ValueError):
        DeviceObjects(0x1000, [[(0, 16)]], sha1=True, crc32=False, copy_to=0x100000)


def test_default_copy_offsets():
    """Objects back to back, every start rounded up to 256 bytes; an object without extents takes no
    room; the room needed ends with the last object's last byte."""
    from efes_amd.batch import COPY_ALIGN, default_copy_offsets
    assert COPY_ALIGN == 256
    objects = [[(7, 1), (100, 300)], [], [(0, 256)], [(5, 0), (9, 257), (1 << 20, 65536 + 3)], [(3, 5)]]
    sizes = np.array([sum(n for _, n in o) for o in objects], dtype=np.int64)
    want, at = [], 0
    for s in sizes:
        at = -(-at // 256) * 256
        want.append(at)
        at += int(s)
    # 301 -> 512; the empty object shares its successor's start; 768 + 65 796 = 66 564 -> 66 816
    assert want == [0, 512, 512, 768, 66816]
    offsets, room = default_copy_offsets(objects)
    assert offsets.dtype == np.uint64 and offsets.tolist() == want
    assert room == want[-1] + 5 == at
    assert (offsets % 256 == 0).all()
    # no two objects' ranges overlap
    ends = offsets.astype(np.int64) + sizes
    assert (ends[:-1] <= offsets[1:].astype(np.int64)).all()
    empty, room0 = default_copy_offsets([])
    assert empty.size == 0 and room0 == 0
