"""efes_objects_order_host and efes_objects_jobs_ordered_host without a GPU, against numpy.

The reference order is np.argsort(~sizes, kind="stable") over uint64 sizes, the sizes as the builder computes them:
E[bound(first[i + 1])] - E[bound(first[i])] modulo 2^64 with first[] clamped to [0, nextents].  The reference of the
ordered build is the table-order expectation of test_objects_jobs_host.py, permuted: slot k of rank r holds the
record of extent first[order[r]] + (k - J[r]).  The GPU tests (test_gpu_objects_order.py) share the tables, the
references and the guard-word harness below.  Bit-exact."""
import ctypes
import random

import numpy as np
import pytest

from efes_amd._lib import JOB_DTYPE, Objects, ObjectsOut
from test_objects_jobs_host import (BASES, HASHES, SENTINEL, U64, Guarded, describe, edge_tables, expectation, make_table,
                                    option_grid, ragged_objects, run_host, table_of)

GUARD32 = 8
SENTINEL32 = np.uint32(0xA5C3A5C3)
TOP = 1 << 20


class Guarded32:
    """A host array of `words` 32-bit words with GUARD32 sentinel words on either side, all of it pre-filled."""

    def __init__(self, words):
        self.words = words
        self.buf = np.full(words + 2 * GUARD32, SENTINEL32, dtype=np.uint32)

    @property
    def ptr(self):
        return self.buf.ctypes.data + 4 * GUARD32

    def body(self):
        return self.buf[GUARD32:GUARD32 + self.words]

    def guards_intact(self):
        return bool((self.buf[:GUARD32] == SENTINEL32).all() and (self.buf[GUARD32 + self.words:] == SENTINEL32).all())

    def untouched(self):
        return bool((self.buf == SENTINEL32).all())


# ---- references
def sizes_of(ext, first):
    """uint64 sizes modulo 2^64, first[] clamped to [0, nextents] (any first[])."""
    n = len(ext)
    with np.errstate(over="ignore"):
        E = np.concatenate((np.zeros(1, U64), np.cumsum(np.asarray(ext, dtype=U64).reshape(n, 2)[:, 1], dtype=U64)))  # stays uint64
        b = np.minimum(np.asarray(first, dtype=np.int64), n)
        return (E[b[1:]] - E[b[:-1]]).astype(U64)


def reference_order(ext, first):
    return np.argsort(~sizes_of(ext, first), kind="stable").astype(np.uint32)


def slots_of(first, order):
    """(jmap, J) of a well-formed table: the table extent of every slot, and the nobjects + 1 slot boundaries."""
    f = np.asarray(first, dtype=np.int64)
    cnt = (f[1:] - f[:-1])[order.astype(np.int64)]
    J = np.concatenate(([0], np.cumsum(cnt)))
    jmap = np.repeat(f[order.astype(np.int64)] - J[:-1], cnt) + np.arange(int(J[-1]), dtype=np.int64)
    return jmap, J.astype(np.uint32)


def ordered_expectation(ext, first, order, **opts):
    """expectation() permuted: jobs, dst, ckpt in slot order, the unchanged layout, job_first."""
    jobs, dst, ck, layout = expectation(ext, first, **opts)
    jmap, J = slots_of(first, order)
    return jobs[jmap], None if dst is None else dst[jmap], None if ck is None else ck[jmap], layout, J


def lengths_table(lengths, seed=1):
    """One extent per object, so the sizes are the lengths."""
    rng = random.Random(seed)
    ext = np.array([(rng.randrange(0, 1 << 30), int(x)) for x in lengths], dtype=U64).reshape(len(lengths), 2)
    return ext, np.arange(len(lengths) + 1, dtype=np.uint32)


def one_byte_lengths(n, byte, seed):
    """n lengths that differ in byte `byte` only (and do differ there)."""
    rng = np.random.default_rng(seed)
    base = U64(rng.integers(0, 1 << 63, dtype=np.uint64)) & ~(U64(0xFF) << U64(8 * byte))
    return base | (rng.integers(0, 256, n, dtype=np.uint64) << U64(8 * byte))


def order_tables():
    """name -> (ext, first): every shape of the issue's list."""
    rng = np.random.default_rng(77)
    t = {}
    for k, objects in enumerate((ragged_objects(), ragged_objects(seed=9, nobjects=300, most=7), ragged_objects(seed=4, nobjects=33, least=1))):
        t[f"random{k}"] = table_of(objects)
    t["random_64bit"] = lengths_table(rng.integers(0, 1 << 64, 500, dtype=np.uint64, endpoint=False))
    t["all_equal"] = lengths_table([4096] * 333)
    t["all_equal_multi"] = table_of([[(0, 100), (7, 200)]] * 50)
    for byte in range(8):
        t[f"byte{byte}"] = lengths_table(one_byte_lengths(400, byte, 100 + byte))
    big = (1 << 63)
    t["wrapping"] = table_of([[(0, big + 5), (1, big + 9)], [(2, 3)], [(3, (1 << 64) - 1), (4, 2)], [(5, big), (6, big), (7, 14)], [(8, 1)],
                              [(9, (1 << 64) - 1)]])
    t["no_extents"] = table_of([[], [(0, 5)], [], [], [(1, 9), (2, 1)], [], [(3, 5)], []])
    t["all_objects_empty"] = table_of([[], [], [], []])
    t["zero_length_extents"] = table_of([[(0, 0)], [(1, 0), (2, 0)], [(3, 7)], [(4, 0), (5, 0), (6, 0)], [], [(7, 0), (8, 7)]])
    asc = np.sort(rng.integers(0, 1 << 40, 700, dtype=np.uint64))
    t["already_sorted"] = lengths_table(asc[::-1])
    t["reverse_sorted"] = lengths_table(asc)
    t["one_object"] = table_of([[(0, 9), (1, 9)]])
    t["heavy_ties"] = lengths_table(rng.choice(np.array([0, 1, 255, 256, 65536, 1 << 24, (1 << 32) + 1, 77], dtype=np.uint64), 5000))
    return t


def malformed(first, n, how):
    first = np.array(first, dtype=np.uint32)
    m = len(first) - 1
    if how == "swap":
        a, b = m // 7, m // 2
        first[a], first[b] = first[b], first[a]
    elif how == "first0":
        first[0] = 3
    elif how == "last_short":
        first[m] = max(n - 4, 0)
    elif how == "last_long":
        first[m] = n + 1000
    elif how == "huge":
        first[m // 2] = 0xFFFFFFFF
    elif how == "random":
        first = np.random.default_rng(3).integers(0, 2 * n + 2, m + 1, dtype=np.uint32)
    else:  # decreasing
        first = first[::-1].copy()
    return first


MALFORMED = ["swap", "first0", "last_short", "last_long", "huge", "random", "decreasing"]


# ---- the calls
def run_order_host(efes_lib, ext, first):
    ext = np.ascontiguousarray(ext, dtype=U64)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    t = Objects(extents=ext.ctypes.data if len(ext) else None, first=first.ctypes.data, nobjects=len(first) - 1, nextents=len(ext))
    G = Guarded32(len(first) - 1)
    return efes_lib.lib().efes_objects_order_host(ctypes.byref(t), G.ptr), G


def run_ordered_host(efes_lib, ext, first, order, *, layout=True, job_first=True, **opts):
    """efes_objects_jobs_ordered_host over guarded outputs: (rc, jobs, dst, ckpt, layout, job_first)."""
    n, m = len(ext), len(first) - 1
    copy = opts.get("copy")
    ext = np.ascontiguousarray(ext, dtype=U64)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    order = np.ascontiguousarray(order, dtype=np.uint32)
    offs = np.ascontiguousarray(copy[1], dtype=U64) if copy is not None and copy[0] == "explicit" else None
    t = make_table(ext, first, offsets_ptr=None if offs is None else offs.ctypes.data, **opts)
    J = Guarded(7 * n)
    D = Guarded(n) if copy is not None else None
    C = Guarded(n) if opts.get("ckpt") else None
    Y = Guarded(m + 1) if layout else None
    F = Guarded32(m + 1) if job_first else None
    out = ObjectsOut(jobs=J.ptr, dst=D.ptr if D else None, ckpt=C.ptr if C else None, layout=Y.ptr if Y else None)
    rc = efes_lib.lib().efes_objects_jobs_ordered_host(ctypes.byref(t), ctypes.byref(out), order.ctypes.data if m else None,
                                                       F.ptr if F else None)
    return rc, J, D, C, Y, F


def check_ordered(got, want, what=""):
    J, D, C, Y, F = got
    jobs, dst, ck, layout, jf = want
    assert J.guards_intact() and (J.body() == jobs.view(U64)).all(), (what, "jobs", np.nonzero(J.body() != jobs.view(U64))[0][:8])
    if D is not None:
        assert D.guards_intact() and (D.body() == dst).all(), (what, "dst")
    if C is not None:
        assert C.guards_intact() and (C.body() == ck).all(), (what, "ckpt")
    if Y is not None:
        assert Y.guards_intact() and (Y.body() == layout).all(), (what, "layout")
    if F is not None:
        assert F.guards_intact() and (F.body() == jf).all(), (what, "job_first", F.body()[:8], jf[:8])


def check_in_range(ext, m, J, D, C, F, bases=BASES):
    """Every address of a job array built from a malformed table or order lies inside its array: the states by an
    object index below m, the sum, status, record, data and length all by ONE extent index below n."""
    n = len(ext)
    jobs = J.body().view(JOB_DTYPE)
    rel = jobs["sum"] - U64(bases["sums"])
    assert (rel % U64(24) == 0).all() and (rel // U64(24) < U64(n)).all()
    j = (rel // U64(24)).astype(np.int64)
    assert (jobs["status"] == U64(bases["status"]) + j.astype(U64) * U64(4)).all()
    assert (jobs["data"] == U64(bases["data"]) + ext[j, 0]).all() and (jobs["length"] == ext[j, 1]).all()
    for field, stride in (("sha1", 104), ("crc32", 4)):
        rel = jobs[field] - U64(bases[field])
        assert (rel % U64(stride) == 0).all() and (rel // U64(stride) < U64(max(m, 1))).all(), field
    assert (jobs["_reserved"] == 0).all() and (jobs["flags"] & ~np.uint32(0xB) == 0).all()
    if C is not None:
        assert (C.body() == U64(bases["ckpt"]) + j.astype(U64) * U64(112)).all()
    if F is not None:
        f = F.body().astype(np.int64)
        assert f[0] == 0 and (np.diff(f) >= 0).all() and f[-1] <= n
    assert all(g is None or g.guards_intact() for g in (J, D, C, F))


# ---- the order
@pytest.mark.parametrize("name", list(order_tables()))
def test_order_matches_numpy(efes_lib, name):
    ext, first = order_tables()[name]
    rc, G = run_order_host(efes_lib, ext, first)
    assert rc == 0 and G.guards_intact()
    want = reference_order(ext, first)
    assert (G.body() == want).all(), (name, G.body()[:16], want[:16])
    if name.startswith("all_") or name == "already_sorted":
        assert (G.body() == np.arange(len(first) - 1)).all()
    if name == "reverse_sorted":
        sizes = sizes_of(ext, first)
        assert (np.diff(sizes[G.body()].astype(np.float64)) <= 0).all()


def test_the_reference_is_longest_first_with_ties_by_index():
    ext, first = order_tables()["heavy_ties"]
    sizes, order = sizes_of(ext, first), reference_order(ext, first)
    pairs = list(zip((-sizes[order].astype(object)).tolist(), order.tolist()))
    assert pairs == sorted(pairs) and len(set(sizes.tolist())) == 8


@pytest.mark.parametrize("how", MALFORMED)
def test_a_malformed_table_still_gives_a_permutation(efes_lib, how):
    ext, first = table_of(ragged_objects(seed=21))
    first = malformed(first, len(ext), how)
    rc, G = run_order_host(efes_lib, ext, first)
    assert rc == 0 and G.guards_intact()
    assert sorted(G.body().tolist()) == list(range(len(first) - 1))
    assert (G.body() == reference_order(ext, first)).all(), how


def test_order_without_extents_or_objects(efes_lib):
    rc, G = run_order_host(efes_lib, np.zeros((0, 2), U64), np.zeros(6, np.uint32))
    assert rc == 0 and G.body().tolist() == [0, 1, 2, 3, 4] and G.guards_intact()
    G = Guarded32(4)
    t = Objects(nobjects=0, nextents=0)
    assert efes_lib.lib().efes_objects_order_host(ctypes.byref(t), G.ptr) == 0 and G.untouched()
    assert efes_lib.lib().efes_objects_order_host(ctypes.byref(t), None) == 0  # nothing is needed for no objects


def test_order_argument_errors(efes_lib):
    L = efes_lib.lib()
    ext, first = table_of(ragged_objects())
    ext, first = np.ascontiguousarray(ext), np.ascontiguousarray(first)
    G = Guarded32(len(first) + 4)

    def call(order=G.ptr, null_in=False, **spoil):
        t = Objects(extents=ext.ctypes.data, first=first.ctypes.data, nobjects=len(first) - 1, nextents=len(ext))
        for k, v in spoil.items():
            setattr(t, k, v)
        return L.efes_objects_order_host(None if null_in else ctypes.byref(t), order)

    assert call() == 0
    G.buf[:] = SENTINEL32
    bad = [dict(null_in=True), dict(nobjects=TOP + 1), dict(nextents=TOP + 1), dict(first=None), dict(order=None),
           dict(order=G.ptr + 1), dict(order=G.ptr + 2), dict(extents=None), dict(extents=None, nobjects=0)]
    for kw in bad:
        assert call(**kw) == efes_lib.EFES_ERR_ARG, kw
        assert G.untouched(), kw
    assert call(extents=None, nextents=0) == 0  # no extents: none are needed


# ---- the ordered build
@pytest.mark.parametrize("hashes", list(HASHES))
def test_identity_order_equals_the_builder(efes_lib, hashes):
    """Over the option grid of the builder's host test: byte for byte efes_objects_jobs_host, and job_first = first."""
    objects = ragged_objects()
    ext, first = table_of(objects)
    ident = np.arange(len(objects), dtype=np.uint32)
    for opts in option_grid(len(objects)):
        opts.update(HASHES[hashes])
        rc, *got = run_ordered_host(efes_lib, ext, first, ident, **opts)
        hrc, *want = run_host(efes_lib, ext, first, **opts)
        assert rc == 0 and hrc == 0, describe(opts)
        for g, h in zip(got[:4], want):
            assert (g is None) == (h is None) and (g is None or (g.guards_intact() and g.body().tobytes() == h.body().tobytes())), describe(opts)
        assert got[4].guards_intact() and (got[4].body() == first).all()


@pytest.mark.parametrize("name", list(edge_tables()))
def test_identity_order_on_the_edge_tables(efes_lib, name):
    ext, first = table_of(edge_tables()[name])
    for opts in option_grid(len(first) - 1):
        rc, *got = run_ordered_host(efes_lib, ext, first, np.arange(len(first) - 1, dtype=np.uint32), **opts)
        hrc, *want = run_host(efes_lib, ext, first, **opts)
        assert rc == 0 and hrc == 0, (name, describe(opts))
        for g, h in zip(got[:4], want):
            assert (g is None) == (h is None) and (g is None or (g.guards_intact() and g.body().tobytes() == h.body().tobytes())), (name, describe(opts))
        assert got[4].guards_intact() and (got[4].body() == first).all(), name


@pytest.mark.parametrize("name", ["ragged", "empty_runs", "zero_lengths", "long", "empty_first", "empty_last"])
def test_a_permutation_moves_whole_objects(efes_lib, name):
    """Slot k holds the table-order record of its (i, j); dst and ckpt likewise; the layout is the table's."""
    ext, first = table_of(edge_tables()[name])
    m = len(first) - 1
    rng = np.random.default_rng(len(name))
    orders = [rng.permutation(m).astype(np.uint32), np.arange(m, dtype=np.uint32)[::-1].copy(), reference_order(ext, first)]
    for order in orders:
        for opts in option_grid(m):
            rc, *got = run_ordered_host(efes_lib, ext, first, order, **opts)
            assert rc == 0
            check_ordered(got, ordered_expectation(ext, first, order, **opts), (name, describe(opts)))


def test_outputs_not_asked_for_are_not_needed(efes_lib):
    ext, first = table_of(ragged_objects(seed=8))
    order = reference_order(ext, first)
    rc, J, D, C, Y, F = run_ordered_host(efes_lib, ext, first, order, layout=False, job_first=False)
    assert rc == 0 and D is C is Y is F is None
    check_ordered((J, D, C, Y, F), ordered_expectation(ext, first, order))
    rc, *got = run_ordered_host(efes_lib, ext, first, order, copy=("default", 16), ckpt=True, layout=False)
    assert rc == 0
    check_ordered(got, ordered_expectation(ext, first, order, copy=("default", 16), ckpt=True))


def test_ordered_without_extents(efes_lib):
    """No job is written; job_first is all zeros and the layout the builder's; first[] and order[] may be anything."""
    for m in (0, 3):
        Y, F = Guarded(m + 1), Guarded32(m + 1)
        order = np.arange(m, dtype=np.uint32)[::-1].copy()
        t = Objects(nobjects=m, nextents=0)
        out = ObjectsOut(layout=Y.ptr)
        assert efes_lib.lib().efes_objects_jobs_ordered_host(ctypes.byref(t), ctypes.byref(out), order.ctypes.data if m else None, F.ptr) == 0
        assert Y.guards_intact() and F.guards_intact() and not Y.body().any() and not F.body().any()


@pytest.mark.parametrize("how", MALFORMED)
def test_a_malformed_table_gives_in_range_jobs(efes_lib, how):
    ext, first = table_of(ragged_objects(seed=21))
    n, m = len(ext), len(first) - 1
    first = malformed(first, n, how)
    rco, G = run_order_host(efes_lib, ext, first)
    for order in (G.body().copy(), np.arange(m, dtype=np.uint32)):
        for copy in (("default", 256), ("explicit", np.arange(m, dtype=U64) * U64(4096))):
            rc, J, D, C, Y, F = run_ordered_host(efes_lib, ext, first, order, ckpt=True, copy=copy, flags=1)
            assert rc == 0 and Y.guards_intact()
            check_in_range(ext, m, J, D, C, F)


@pytest.mark.parametrize("how", ["constant", "out_of_range", "random", "duplicates"])
def test_an_order_that_is_no_permutation_gives_in_range_jobs(efes_lib, how):
    ext, first = table_of(ragged_objects(seed=22))
    n, m = len(ext), len(first) - 1
    rng = np.random.default_rng(8)
    order = {"constant": np.full(m, int(np.argmax(np.diff(first.astype(np.int64)))), np.uint32),
             "out_of_range": np.full(m, 0xFFFFFFFF, np.uint32),
             "random": rng.integers(0, 1 << 32, m, dtype=np.uint32),
             "duplicates": rng.integers(0, m, m, dtype=np.uint32)}[how]
    rc, J, D, C, Y, F = run_ordered_host(efes_lib, ext, first, order, ckpt=True, copy=("default", 256), flags=1)
    assert rc == 0 and Y.guards_intact()
    check_in_range(ext, m, J, D, C, F)


def test_ordered_argument_errors(efes_lib):
    """The builder's errors and the order's own; a refused call leaves every output's sentinels alone."""
    L = efes_lib.lib()
    ext, first = table_of(ragged_objects())
    ext, first = np.ascontiguousarray(ext), np.ascontiguousarray(first)
    n, m = len(ext), len(first) - 1
    order = np.arange(m + 1, dtype=np.uint32)
    offs = np.zeros(m, dtype=U64)
    G = dict(jobs=Guarded(7 * n), dst=Guarded(n), ckpt=Guarded(n), layout=Guarded(m + 1))
    F = Guarded32(m + 2)

    def call(order_ptr=order.ctypes.data, jf=F.ptr, null_in=False, null_out=False, out_spoil=(), **spoil):
        t = make_table(ext, first, ckpt=True, copy=("explicit", offs), offsets_ptr=offs.ctypes.data)
        for k, v in spoil.items():
            setattr(t, k, v)
        out = ObjectsOut(**{k: (None if k in out_spoil else g.ptr) for k, g in G.items()})
        return L.efes_objects_jobs_ordered_host(None if null_in else ctypes.byref(t), None if null_out else ctypes.byref(out), order_ptr, jf)

    assert call() == 0
    for g in list(G.values()) + [F]:
        g.buf[:] = SENTINEL if g.buf.dtype == U64 else SENTINEL32
    bad = [dict(null_in=True), dict(null_out=True), dict(nobjects=TOP + 1), dict(nextents=TOP + 1), dict(extents=None),
           dict(first=None), dict(sums=None), dict(out_spoil=("jobs",)), dict(sha1=None, crc32=None), dict(out_spoil=("dst",)),
           dict(out_spoil=("ckpt",)), dict(copy_to=None), dict(flags=4), dict(flags=0x80000000), dict(copy_align=3),
           dict(copy_align=1 << 21), dict(order_ptr=None), dict(order_ptr=order.ctypes.data + 2), dict(jf=F.ptr + 2),
           dict(jf=F.ptr + 1)]
    for kw in bad:
        assert call(**kw) == efes_lib.EFES_ERR_ARG, kw
        assert all(g.untouched() for g in G.values()) and F.untouched(), kw
    assert call(jf=None) == 0 and F.untouched()
