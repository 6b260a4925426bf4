"""The chained CRC's C ABI (efes_crc32_chain) without a GPU: the flag, the scratch size, the argument
error that needs no device, and the ABI version, which the purely additive call leaves at 8."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")


def _header_constant(name: str) -> int:
    m = re.search(r"#define\s+%s\s+(\w+)" % name, open(HEADER).read())
    assert m, name
    return int(re.sub(r"u$", "", m.group(1)), 0)


def test_flag_is_0x8_in_header_and_binding(efes_lib):
    assert _header_constant("EFES_JOB_CHAIN") == 0x8 == efes_lib.EFES_JOB_CHAIN
    others = [efes_lib.EFES_JOB_FINALIZE, efes_lib.EFES_JOB_INIT, efes_lib.EFES_JOB_SUM_ONLY]
    assert all(efes_lib.EFES_JOB_CHAIN & f == 0 for f in others)


def test_scratch_size(efes_lib):
    f, batch = efes_lib.lib().efes_crc32_chain_scratch, efes_lib.lib().efes_crc32_batch_scratch
    MAX = efes_lib.EFES_CRC_BATCH_MAX_JOBS
    assert f(0) == 0 and f(MAX + 1) == 0 and f(0xFFFFFFFF) == 0
    counts = (1, 2, 1023, 1024, 1025, 65537, MAX)
    sizes = [f(n) for n in counts]
    assert all(s > 0 for s in sizes), sizes
    assert sizes == sorted(sizes), sizes
    assert all(s >= batch(n) for s, n in zip(sizes, counts)), sizes
    # the batch scratch plus one 16-byte element per job and per block of 1024 jobs
    assert [s - batch(n) for s, n in zip(sizes, counts)] == [16 * (n + (n + 1023) // 1024) for n in counts]
    from efes_amd import hashing
    assert hashing.crc32_chain_scratch(1025) == sizes[4]


def test_null_context_is_an_argument_error(efes_lib):
    L = efes_lib.lib()
    assert L.efes_crc32_chain(None, None, 0, None, 0, None) == efes_lib.EFES_ERR_ARG
    job = efes_lib.Job()
    assert L.efes_crc32_chain(None, ctypes.addressof(job), 1, None, 0, None) == efes_lib.EFES_ERR_ARG


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8 == _header_constant("EFES_ABI_VERSION")
