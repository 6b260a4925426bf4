"""efes_objects_results_host without a GPU: the sums and statuses a chain call leaves per extent, sorted out per
object -- one 32-byte result (sum, status, verdict), the ascending list of the objects that are not in order, four
counters -- against expectation(), the rules of efes_hash.h "Object results" in vectorised numpy.

The function touches no data, so the sums are random bytes and the statuses random picks of {0, 0, 0, -2, -4, -99}.
Every output lies between sentinel words; the inputs are numpy arrays of exactly the table's size.  A table that
breaks the rules must come back EFES_OK with nothing outside the outputs written; that no input is read out of
range is what the standalone sanitizer program (tests/cpp/objects_results_invalid.cpp) checks, over heap arrays
of exact size.  The GPU tests (test_gpu_objects_results.py) share the tables, the expectation and the harness.
Bit-exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from efes_amd._lib import (EFES_HASH_CRC32, EFES_HASH_SHA1, EFES_VERDICT_EMPTY, EFES_VERDICT_FAILED, EFES_VERDICT_MISMATCH,
                           EFES_VERDICT_OK, OBJECT_RESULT_DTYPE, Objects, Results)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8  # 32-bit sentinel words on either side of every output array (32 bytes: the records stay 8-byte aligned)
SENTINEL = np.uint32(0xA5C3A5C3)
STATUSES = np.array([0, 0, 0, -2, -4, -99], dtype=np.int32)
COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2051]
MASKS = [0, EFES_HASH_SHA1, EFES_HASH_CRC32, EFES_HASH_SHA1 | EFES_HASH_CRC32]


# ---- the rules, in numpy
def expectation(first, status, sums, expected=None, compare=3):
    """(records, bad, counts) for a WELL-FORMED table: first (nobjects + 1), status (n) int32, sums (n, 24) uint8,
    expected (nobjects, 24) uint8 or None."""
    m, n = len(first) - 1, len(status)
    f = first.astype(np.int64)
    count = f[1:] - f[:-1]
    owner = np.repeat(np.arange(m, dtype=np.int64), count)  # of every extent
    failed = np.nonzero(status != 0)[0]
    fail = np.full(m, n, dtype=np.int64)  # the lowest failing member of each object, n: none
    np.minimum.at(fail, owner[failed], failed)
    rec = np.zeros(m, dtype=OBJECT_RESULT_DTYPE)
    has = count > 0
    last = np.where(has, f[1:] - 1, 0)
    st, su = np.append(status, np.int32(0)), np.concatenate((sums.reshape(n, 24), np.zeros((1, 24), np.uint8)))
    rec["status"] = np.where(has, st[fail], 0)
    keep = has & (st[np.where(has, last, n)] == 0)  # the last member wrote a sum
    rec["sum"] = np.where(keep[:, None], su[np.where(keep, last, n)], 0)
    ok = has & (rec["status"] == 0)
    differs = np.zeros(m, dtype=bool)
    if expected is not None:
        d = rec["sum"] != np.asarray(expected).reshape(m, 24)
        if compare & EFES_HASH_SHA1:
            differs |= d[:, :20].any(axis=1)
        if compare & EFES_HASH_CRC32:
            differs |= d[:, 20:].any(axis=1)
    rec["verdict"] = np.where(~has, EFES_VERDICT_EMPTY, np.where(~ok, EFES_VERDICT_FAILED,
                                                                np.where(differs, EFES_VERDICT_MISMATCH, EFES_VERDICT_OK)))
    bad = np.nonzero((rec["verdict"] == EFES_VERDICT_MISMATCH) | (rec["verdict"] == EFES_VERDICT_FAILED))[0].astype(np.uint32)
    return rec, bad, np.bincount(rec["verdict"], minlength=4).astype(np.uint32)


# ---- the harness
class Guarded:
    """A host output array of `words` 32-bit words with GUARD sentinel words on either side, all of it pre-filled
    with the sentinel."""

    def __init__(self, words):
        self.words = words
        self.buf = np.full(words + 2 * GUARD, SENTINEL, dtype=np.uint32)

    @property
    def ptr(self):
        return self.buf.ctypes.data + 4 * GUARD

    def body(self):
        return self.buf[GUARD:GUARD + self.words]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all() and (self.buf[GUARD + self.words:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def make_request(m, *, expected_ptr=None, compare=3, results=True, bad=True, counts=True, guarded=Guarded):
    """(efes_results, R, B, C): the request over fresh guarded outputs (None: passed as NULL)."""
    R = guarded(8 * m) if results else None
    B = guarded(m) if bad else None
    C = guarded(4) if counts else None
    req = Results(expected=expected_ptr, compare=compare, results=R.ptr if R else None, bad=B.ptr if B else None,
                  counts=C.ptr if C else None)
    return req, R, B, C


def make_table(first_ptr, sums_ptr, status_ptr, m, n):
    """Only first, sums, status and the two counts are read; every other field stays NULL."""
    return Objects(first=first_ptr, sums=sums_ptr, status=status_ptr, nobjects=m, nextents=n)


def run_host(efes_lib, first, status, sums, expected=None, compare=3, **outs):
    first = np.ascontiguousarray(first, dtype=np.uint32)
    status = np.ascontiguousarray(status, dtype=np.int32)
    sums = np.ascontiguousarray(sums, dtype=np.uint8)
    m, n = len(first) - 1, len(status)
    exp = None if expected is None else np.ascontiguousarray(expected, dtype=np.uint8)
    t = make_table(first.ctypes.data, sums.ctypes.data if n else None, status.ctypes.data if n else None, m, n)
    req, R, B, C = make_request(m, expected_ptr=(exp.ctypes.data if m else None) if exp is not None else None, compare=compare, **outs)
    rc = efes_lib.lib().efes_objects_results_host(ctypes.byref(t), ctypes.byref(req))
    return rc, R, B, C


def check_outputs(got, want, what=""):
    """got: (R, B, C) Guarded or None; want: expectation()'s tuple.  Bodies equal, guards intact, nothing behind
    the list's end."""
    R, B, C = got
    rec, bad, counts = want
    if R is not None:
        assert R.guards_intact(), (what, "results guards")
        g = R.body().view(OBJECT_RESULT_DTYPE)
        assert g.tobytes() == rec.tobytes(), (what, "results", np.nonzero(g != rec)[0][:8])
    if B is not None:
        assert B.guards_intact(), (what, "bad guards")
        assert (B.body()[:len(bad)] == bad).all(), (what, "bad", B.body()[:8], bad[:8])
        assert (B.body()[len(bad):] == SENTINEL).all(), (what, "something behind the bad list")
    assert C.guards_intact() and (C.body() == counts).all(), (what, "counts", C.body(), counts)
    assert int(counts[1]) + int(counts[2]) == len(bad)


# ---- tables and inputs
def first_of(counts):
    return np.concatenate(([0], np.cumsum(np.asarray(counts, dtype=np.int64)))).astype(np.uint32)


def random_first(m, n, rng):
    """m objects over n extents: random boundaries, so some objects are empty."""
    if m == 0:
        return np.array([0], dtype=np.uint32)  # (the extents then have no owner; only n == 0 is well-formed)
    return np.concatenate(([0], np.sort(rng.integers(0, n + 1, m - 1)), [n])).astype(np.uint32)


def random_inputs(n, rng, statuses=True):
    status = rng.choice(STATUSES, n).astype(np.int32) if statuses else np.zeros(n, np.int32)
    return status, rng.integers(0, 256, (n, 24), dtype=np.uint8)


def own_sums(first, status, sums):
    """The expected digests that match: every object's last sum as the call reports it."""
    return expectation(first, status, sums)[0]["sum"].copy()


def edge_tables():
    return {
        "empty_first": first_of([0, 0, 0, 2, 1, 3]),
        "empty_last": first_of([1, 3, 2, 0, 0, 0]),
        "empty_runs": first_of([0, 0, 1, 0, 0, 0, 2, 0, 1, 0, 0, 4, 0]),
        "all_empty": first_of([0, 0, 0]),
        "no_objects": first_of([]),
        "one_object": first_of([300]),
        "one_object_one_extent": first_of([1]),
        "one_extent_each": first_of([1] * 300),
    }


# ---- the tests
@pytest.mark.parametrize("nobjects", COUNTS)
def test_counts_in_combination(efes_lib, nobjects):
    rng = np.random.default_rng(100 + nobjects)
    for n in COUNTS:
        if nobjects == 0 and n:
            continue  # extents without an object: not a well-formed table (test_invalid_tables)
        first = random_first(nobjects, n, rng)
        status, sums = random_inputs(n, rng)
        exp = own_sums(first, status, sums)
        spoil = rng.random(nobjects) < 0.3
        exp[spoil, rng.integers(0, 24, int(spoil.sum()))] ^= 0x40
        for compare in MASKS:
            rc, *got = run_host(efes_lib, first, status, sums, exp, compare)
            assert rc == 0
            check_outputs(got, expectation(first, status, sums, exp, compare), (nobjects, n, compare))


@pytest.mark.parametrize("name", list(edge_tables()))
def test_edge_tables(efes_lib, name):
    first = edge_tables()[name]
    n = int(first[-1])
    rng = np.random.default_rng(7)
    for statuses in (False, True):
        status, sums = random_inputs(n, rng, statuses)
        exp = own_sums(first, status, sums)
        rc, *got = run_host(efes_lib, first, status, sums, exp, 3)
        assert rc == 0
        want = expectation(first, status, sums, exp, 3)
        check_outputs(got, want, (name, statuses))
        assert want[2][1] == 0  # nothing differs from its own sum
        if not statuses:
            assert want[2][2] == 0 and len(want[1]) == 0


@pytest.mark.parametrize("where", ["last", "first", "middle"])
def test_failure_placement(efes_lib, where):
    """One failing member per object: the last (no sum was written: zeros), the first or only a middle one (the last
    member is EFES_OK, so its sum is reported beside the failure)."""
    counts = [5, 1, 3, 7, 2, 64, 3]
    first = first_of(counts)
    n = int(first[-1])
    rng = np.random.default_rng(3)
    status, sums = np.zeros(n, np.int32), rng.integers(1, 256, (n, 24), dtype=np.uint8)
    hit = [i for i, c in enumerate(counts) if c >= 3 and i != 3]  # object 3 stays whole
    for i in hit:
        at = {"last": first[i + 1] - 1, "first": first[i], "middle": first[i] + counts[i] // 2}[where]
        status[at] = -4
    rc, R, B, C = run_host(efes_lib, first, status, sums, own_sums(first, status, sums), 3)
    assert rc == 0
    want = expectation(first, status, sums, own_sums(first, status, sums), 3)
    check_outputs((R, B, C), want, where)
    rec = R.body().view(OBJECT_RESULT_DTYPE)
    assert B.body()[:len(hit)].tolist() == hit and C.body().tolist() == [len(counts) - len(hit), 0, len(hit), 0]
    for i in hit:
        assert rec["status"][i] == -4 and rec["verdict"][i] == EFES_VERDICT_FAILED
        assert (rec["sum"][i] == 0).all() if where == "last" else (rec["sum"][i] == sums[first[i + 1] - 1]).all()
    # the FIRST failing member's status, whatever fails behind it
    status[first[3] + 2], status[first[3] + 4] = -2, -99
    rc, R, B, C = run_host(efes_lib, first, status, sums)
    assert rc == 0 and R.body().view(OBJECT_RESULT_DTYPE)["status"][3] == -2


@pytest.mark.parametrize("offset", [0, 19, 20, 23])
def test_one_differing_byte_under_each_mask(efes_lib, offset):
    first = first_of([2, 0, 1, 4, 1])
    n = int(first[-1])
    status, sums = random_inputs(n, np.random.default_rng(offset), statuses=False)
    exp = own_sums(first, status, sums)
    exp[3, offset] ^= 1
    exp[1] = 0xEE  # an object without extents: its entry is not compared
    for compare in MASKS:
        rc, R, B, C = run_host(efes_lib, first, status, sums, exp, compare)
        assert rc == 0
        check_outputs((R, B, C), expectation(first, status, sums, exp, compare), (offset, compare))
        seen = bool(compare & (EFES_HASH_SHA1 if offset < 20 else EFES_HASH_CRC32))
        assert C.body().tolist() == ([3, 1, 0, 1] if seen else [4, 0, 0, 1])
        assert R.body().view(OBJECT_RESULT_DTYPE)["verdict"][3] == (EFES_VERDICT_MISMATCH if seen else EFES_VERDICT_OK)


def test_expected_and_outputs_that_may_be_null(efes_lib):
    rng = np.random.default_rng(17)
    first = random_first(70, 200, rng)
    status, sums = random_inputs(200, rng)
    garbage = rng.integers(0, 256, (70, 24), dtype=np.uint8)
    want = expectation(first, status, sums, None)
    assert want[2][1] == 0
    for compare in MASKS:  # expected == NULL: nothing is compared under any mask
        rc, *got = run_host(efes_lib, first, status, sums, None, compare)
        assert rc == 0
        check_outputs(got, want, compare)
    rc, *got = run_host(efes_lib, first, status, sums, garbage, 0)  # compare == 0: expected is not looked at
    assert rc == 0
    check_outputs(got, want, "compare 0")
    want = expectation(first, status, sums, garbage, 3)
    for outs in (dict(results=False), dict(bad=False), dict(results=False, bad=False)):
        rc, R, B, C = run_host(efes_lib, first, status, sums, garbage, 3, **outs)
        assert rc == 0 and (R is None) == ("results" in outs) and (B is None) == ("bad" in outs)
        check_outputs((R, B, C), want, outs)
    rc, R, B, C = run_host(efes_lib, first, status, sums, garbage, 3, counts=False)  # counts is required
    assert rc == efes_lib.EFES_ERR_ARG and R.untouched() and B.untouched()


def invalid_tables(m=40, n=90, seed=5):
    """name -> first (m + 1): each breaks one rule of a well-formed table."""
    rng = np.random.default_rng(seed)
    good = random_first(m, n, rng)
    out = {}
    out["decreasing"] = good[::-1].copy()
    swap = good.copy()
    swap[[5, 30]] = swap[[30, 5]]
    out["swapped"] = swap
    f0 = good.copy()
    f0[0] = 7
    out["first0"] = f0
    for name, v in (("last_short", n - 9), ("last_long", n + 1000), ("last_top", 0xFFFFFFFF)):
        f = good.copy()
        f[m] = v
        out[name] = f
    near = good.copy()
    near[m // 2], near[m // 2 + 1], near[3] = 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000
    out["near_2_32"] = near
    out["all_top"] = np.full(m + 1, 0xFFFFFFFF, dtype=np.uint32)
    out["random"] = rng.integers(0, 1 << 32, m + 1, dtype=np.uint64).astype(np.uint32)
    return out


@pytest.mark.parametrize("name", list(invalid_tables()))
def test_invalid_tables(efes_lib, name):
    """EFES_OK, and nothing outside the outputs is written; what is written is not compared."""
    first = invalid_tables()[name]
    m, n = len(first) - 1, 90
    rng = np.random.default_rng(1)
    status, sums = random_inputs(n, rng)
    exp = rng.integers(0, 256, (m, 24), dtype=np.uint8)
    rc, R, B, C = run_host(efes_lib, first, status, sums, exp, 3)
    assert rc == 0 and R.guards_intact() and B.guards_intact() and C.guards_intact()
    rc, R, B, C = run_host(efes_lib, np.array([0], np.uint32), status, sums)  # extents without an object
    assert rc == 0 and C.guards_intact() and C.body().tolist() == [0, 0, 0, 0]


def test_standalone_sanitizer_program(tmp_path):
    """tests/cpp/objects_results_invalid.cpp replays tables that break the rules against efes_objects_results_host on
    heap arrays of exact size, built with -fsanitize=address,undefined together with efes_objects.cpp and the shared
    rules: an out-of-range read or write ends it with a report.  A program of its own with the sanitizer runtimes
    linked in statically: it needs nothing preloaded and runs in the environment it is given, unchanged."""
    exe = tmp_path / "objects_results_invalid"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "objects_results_invalid.cpp"),
           os.path.join(ROOT, "efes_amd", "csrc", "efes_objects.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    missing = [line for line in built.stderr.splitlines() if "cannot find" in line and ("asan" in line or "ubsan" in line)]
    if built.returncode != 0 and missing:
        pytest.skip("the toolchain lacks the static sanitizer runtime: " + missing[0].strip())
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-4000:]
    assert "tables ok" in ran.stdout
