"""The chained SHA-1 + CRC-32 call's C ABI (efes_hash_chain) without a GPU: the symbols, the scratch size,
the argument error that needs no device, the job-count limit, and the ABI version, which the purely
additive call leaves at 8."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")


def _header_constant(name: str) -> int:
    m = re.search(r"#define\s+%s\s+(.+)" % name, open(HEADER).read())
    assert m, name
    return int(eval(re.sub(r"(\d)u\b", r"\1", m.group(1).split("/*")[0])))


def test_symbols_exist(efes_lib):
    L = efes_lib.lib()
    assert L.efes_hash_chain and L.efes_hash_chain_scratch
    assert "efes_hash_chain" in efes_lib.SIGNATURES and "efes_hash_chain_scratch" in efes_lib.SIGNATURES
    header = open(HEADER).read()
    assert re.search(r"\bint\s+efes_hash_chain\s*\(", header) and re.search(r"\bsize_t\s+efes_hash_chain_scratch\s*\(", header)


def test_scratch_size(efes_lib):
    f = efes_lib.lib().efes_hash_chain_scratch
    MAX = efes_lib.EFES_HASH_CHAIN_MAX_JOBS
    assert f(0) == 0 and f(MAX + 1) == 0 and f(0xFFFFFFFF) == 0
    counts = (1, 2, 1023, 1024, 1025, 65537, MAX)
    sizes = [f(n) for n in counts]
    assert all(s > 0 for s in sizes), sizes
    assert sizes == sorted(sizes) and sizes[0] < sizes[2] < sizes[-1], sizes
    from efes_amd import hashing
    assert [hashing.hash_chain_scratch(n) for n in counts] == sizes
    assert hashing.hash_chain_scratch(0) == 0


def test_null_context_is_an_argument_error(efes_lib):
    L = efes_lib.lib()
    assert L.efes_hash_chain(None, None, 0, None, 0, None) == efes_lib.EFES_ERR_ARG
    job = efes_lib.Job()
    assert L.efes_hash_chain(None, ctypes.addressof(job), 1, None, 0, None) == efes_lib.EFES_ERR_ARG


def test_abi_version_stays_8(efes_lib):
    assert efes_lib.lib().efes_abi_version() == 8 == _header_constant("EFES_ABI_VERSION")


def test_max_jobs_in_header_and_binding(efes_lib):
    assert _header_constant("EFES_HASH_CHAIN_MAX_JOBS") == efes_lib.EFES_HASH_CHAIN_MAX_JOBS == 1 << 20
