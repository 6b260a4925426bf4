"""The wide chain walk's C ABI (efes_hash_chain_wide, efes_hash_chain_auto_mode_wide) without a GPU: the
symbols, the argument error that needs no device, and the host-only mode choice -- that it is
efes_hash_chain_auto_mode wherever it is not EFES_MODE_WIDE and stays EFES_MODE_WIDE once it has become it,
not the threshold itself, which a measurement may move (or remove)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")
SWEEP = sorted(set(list(range(0, 20000, 61)) + [1 << k for k in range(25)] + [(1 << k) + 1 for k in range(25)] +
                   [(1 << 20) - 1, 0xFFFFFFFF]))


def test_symbols_exist(efes_lib):
    L = efes_lib.lib()
    assert L.efes_hash_chain_wide and L.efes_hash_chain_auto_mode_wide
    assert "efes_hash_chain_wide" in efes_lib.SIGNATURES and "efes_hash_chain_auto_mode_wide" in efes_lib.SIGNATURES
    header = open(HEADER).read()
    assert re.search(r"\bint\s+efes_hash_chain_wide\s*\(", header)
    assert re.search(r"\bint\s+efes_hash_chain_auto_mode_wide\s*\(", header)


def test_null_context_is_an_argument_error(efes_lib):
    L = efes_lib.lib()
    job = efes_lib.Job()
    assert L.efes_hash_chain_wide(None, None, 0, None, None, 0, None) == efes_lib.EFES_ERR_ARG
    assert L.efes_hash_chain_wide(None, ctypes.addressof(job), 1, None, None, 0, None) == efes_lib.EFES_ERR_ARG


def test_auto_mode_wide_against_auto_mode(efes_lib):
    f, g = efes_lib.lib().efes_hash_chain_auto_mode_wide, efes_lib.lib().efes_hash_chain_auto_mode
    allowed = {efes_lib.MODE_DEEP, efes_lib.MODE_WIDE, *efes_lib.MODE_GROUP.values()}
    for n in range(0, 1025):
        assert f(None, n) == g(None, n), n
    wide = []
    for n in SWEEP:
        m = f(None, n)
        assert m in allowed, (n, m)
        if m != efes_lib.MODE_WIDE:
            assert m == g(None, n), n
        wide.append(m == efes_lib.MODE_WIDE)
    assert all(b or not a for a, b in zip(wide, wide[1:])), "once EFES_MODE_WIDE, EFES_MODE_WIDE for every larger count"


def test_python_agrees_with_c(efes_lib):
    from efes_amd import hashing
    f = efes_lib.lib().efes_hash_chain_auto_mode_wide
    for n in (0, 1, 1024, 1025, 16384, 16385, 32768, 65535, 65536, 65537, 100000, 262144, 1 << 20):
        assert hashing.hash_chain_auto_mode_wide(n) == f(None, n), n


def test_device_objects_wide_needs_sha1():
    from efes_amd import batch
    for walk in ("wide", "auto_wide"):
        with pytest.raises(ValueError):
            batch.DeviceObjects(0, [[(0, 1)]], walk=walk)
