"""The batched CRC's C ABI (efes_crc32_batch, ABI 8) without a GPU: constants, the scratch size, the
argument errors that need no device."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")


def _header_constant(name: str) -> int:
    m = re.search(r"#define\s+%s\s+(.+)" % name, open(HEADER).read())
    assert m, name
    expr = re.sub(r"(?<=\d)u\b", "", m.group(1).split("/*")[0]).strip()
    assert re.fullmatch(r"[\d\s()<]+", expr), expr
    return int(eval(expr))


def test_constants_match_the_binding(efes_lib):
    assert _header_constant("EFES_CRC_BATCH_TILE") == efes_lib.EFES_CRC_BATCH_TILE
    assert _header_constant("EFES_CRC_BATCH_MAX_JOBS") == efes_lib.EFES_CRC_BATCH_MAX_JOBS
    assert efes_lib.EFES_CRC_BATCH_MAX_JOBS >= 1 << 20
    assert efes_lib.EFES_CRC_BATCH_TILE % 16 == 0


def test_scratch_size(efes_lib):
    f = efes_lib.lib().efes_crc32_batch_scratch
    MAX = efes_lib.EFES_CRC_BATCH_MAX_JOBS
    assert f(0) == 0 and f(MAX + 1) == 0 and f(0xFFFFFFFF) == 0
    sizes = [f(n) for n in (1, 2, 1023, 1024, 1025, 65537, MAX)]
    assert all(s > 0 for s in sizes), sizes
    assert sizes == sorted(sizes), sizes
    from efes_amd import hashing
    assert hashing.crc32_batch_scratch(1025) == sizes[4]


def test_null_context_is_an_argument_error(efes_lib):
    L = efes_lib.lib()
    assert L.efes_crc32_batch(None, None, 0, None, 0, None) == efes_lib.EFES_ERR_ARG
    job = efes_lib.Job()
    assert L.efes_crc32_batch(None, ctypes.addressof(job), 1, None, 0, None) == efes_lib.EFES_ERR_ARG


def test_abi_version_is_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8 == _header_constant("EFES_ABI_VERSION")
