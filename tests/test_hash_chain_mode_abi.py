"""The grouped chain walk's C ABI (efes_hash_chain_mode, efes_hash_chain_auto_mode) without a GPU: the
symbols, the argument error that needs no device, and the host-only mode choice -- its endpoints and its
monotonicity, not its thresholds, which a measurement may move."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "efes_hash.h")


def _modes(efes_lib):
    """mode -> lanes per chain (the wave walk: all 64)."""
    return {efes_lib.MODE_DEEP: 64, **{m: g for g, m in efes_lib.MODE_GROUP.items()}}


def test_symbols_exist(efes_lib):
    L = efes_lib.lib()
    assert L.efes_hash_chain_mode and L.efes_hash_chain_auto_mode
    assert "efes_hash_chain_mode" in efes_lib.SIGNATURES and "efes_hash_chain_auto_mode" in efes_lib.SIGNATURES
    header = open(HEADER).read()
    assert re.search(r"\bint\s+efes_hash_chain_mode\s*\(", header)
    assert re.search(r"\bint\s+efes_hash_chain_auto_mode\s*\(", header)


def test_null_context_is_an_argument_error(efes_lib):
    L = efes_lib.lib()
    job = efes_lib.Job()
    modes = _modes(efes_lib)
    assert len(modes) == 5
    for mode in modes:
        assert L.efes_hash_chain_mode(None, None, 0, None, 0, None, mode) == efes_lib.EFES_ERR_ARG, mode
        assert L.efes_hash_chain_mode(None, ctypes.addressof(job), 1, None, 0, None, mode) == efes_lib.EFES_ERR_ARG, mode


def test_auto_mode_endpoints_and_monotonicity(efes_lib):
    f = efes_lib.lib().efes_hash_chain_auto_mode
    modes = _modes(efes_lib)
    for n in (0, 1, 1024):
        assert f(None, n) == efes_lib.MODE_DEEP, n
    for n in (16 * 1024 + 1, 20000, 1 << 20, 0xFFFFFFFF):
        assert f(None, n) == efes_lib.MODE_GROUP[4], n
    sweep = sorted(set(list(range(0, 20000, 61)) + [1 << k for k in range(25)] + [(1 << k) + 1 for k in range(25)]))
    lanes = []
    for n in sweep:
        m = f(None, n)
        assert m in modes, (n, m)
        lanes.append(modes[m])
    assert all(a >= b for a, b in zip(lanes, lanes[1:])), "lanes per chain never increase with the chain count"


def test_python_agrees_with_c(efes_lib):
    from efes_amd import hashing
    f = efes_lib.lib().efes_hash_chain_auto_mode
    for n in (0, 1, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 100000):
        assert hashing.hash_chain_auto_mode(n) == f(None, n), n
