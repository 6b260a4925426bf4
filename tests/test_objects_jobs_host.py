"""efes_objects_jobs_host without a GPU: an object table (extents + object boundaries) expanded into the job
array, the destination pointers, the record pointers and the gather layout, against

  * expectation(): the contract of efes_hash.h "Object tables" in vectorised numpy -- the owner by
    searchsorted(first[:nobjects], j, 'right') - 1, the cumulative sum E of the lengths, the scan of the rounded
    sizes -- and
  * parent_arrays(): the arithmetic of DeviceObjects.__init__ and default_copy_offsets (efes_amd/batch.py) as
    they stood before the builder, lifted here over Python lists: for a well-formed table the three arrays are
    byte for byte what that code uploads.

The builder touches no data bytes, so base addresses and lengths are fictitious.  Every table's total length
stays below 2^63, so Python-int and wrapping arithmetic agree.  The GPU tests (test_gpu_objects_jobs.py) share
the tables, the expectation and the guard-word harness below.  Bit-exact."""
import itertools
import random

import numpy as np
import pytest

from efes_amd._lib import (CHECKPOINT_DTYPE, EFES_JOB_CHAIN, EFES_JOB_FINALIZE, EFES_JOB_INIT, EFES_OBJECTS_FRESH,
                           EFES_OBJECTS_RUNNING, JOB_DTYPE, Objects, ObjectsOut)

GUARD = 4  # 64-bit sentinel words on either side of every output array
SENTINEL = np.uint64(0xA5C3A5C3A5C3A5C3)
U64 = np.uint64

# fictitious base addresses, far apart, so that a pointer formed from the wrong base or index shows
BASES = dict(data=0x7F10_0000_0000, sha1=0x7F20_0000_0000, crc32=0x7F30_0000_0000, sums=0x7F40_0000_0000,
             status=0x7F50_0000_0000, ckpt=0x7F60_0000_0000, copy_to=0x7F70_0000_0000)


def table_of(objects):
    """(ext (n, 2) uint64, first (nobjects + 1) uint32) of a list of lists of (offset, length)."""
    counts = np.array([len(o) for o in objects], dtype=np.int64)
    ext = np.array([e for o in objects for e in o], dtype=np.uint64).reshape(int(counts.sum()), 2)
    return ext, np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)


def objects_of(ext, first):
    return [[(int(o), int(n)) for o, n in ext[int(a):int(b)]] for a, b in zip(first[:-1], first[1:])]


def expectation(ext, first, *, bases=BASES, sha1=True, crc32=True, status=True, ckpt=False, copy=None, flags=0):
    """What the call must write for a WELL-FORMED table.  copy: None, ("default", align) or ("explicit",
    offsets).  Returns jobs, dst, ckpt pointers (None where not asked for) and the layout (nobjects + 1)."""
    n, m = len(ext), len(first) - 1
    j = np.arange(n, dtype=np.int64)
    owner = np.maximum(np.searchsorted(first[:m], j, "right") - 1, 0)
    f64 = first.astype(np.int64)
    jobs = np.zeros(n, dtype=JOB_DTYPE)
    jobs["data"] = U64(bases["data"]) + ext[:, 0]
    jobs["length"] = ext[:, 1]
    if sha1:
        jobs["sha1"] = U64(bases["sha1"]) + owner.astype(U64) * U64(104)
    if crc32:
        jobs["crc32"] = U64(bases["crc32"]) + owner.astype(U64) * U64(4)
    jobs["sum"] = U64(bases["sums"]) + j.astype(U64) * U64(24)
    if status:
        jobs["status"] = U64(bases["status"]) + j.astype(U64) * U64(4)
    if n:
        head, last = j == f64[owner], j + 1 == f64[owner + 1]
        fl = np.where(head, EFES_JOB_INIT if flags & EFES_OBJECTS_FRESH else 0, EFES_JOB_CHAIN).astype(np.uint32)
        fl[last | bool(flags & EFES_OBJECTS_RUNNING)] |= np.uint32(EFES_JOB_FINALIZE)
        jobs["flags"] = fl
    E = np.concatenate(([0], np.cumsum(ext[:, 1], dtype=U64))).astype(U64)
    size = E[f64[1:]] - E[f64[:-1]]
    if copy is not None and copy[0] == "explicit":
        L = np.asarray(copy[1], dtype=U64)
        room = int((L + size).max()) if m else 0
    else:
        a = U64(copy[1] if copy else 256)
        rounded = (size + (a - U64(1))) & ~(a - U64(1))
        L = (np.cumsum(rounded, dtype=U64) - rounded).astype(U64)
        room = int(L[-1] + size[-1]) if m else 0
    layout = np.concatenate((L, [room])).astype(U64)
    dst = None
    if copy is not None:
        dst = (U64(bases["copy_to"]) + L[owner] + (E[:-1] - E[f64[owner]])).astype(U64) if n else np.zeros(0, U64)
    ck = U64(bases["ckpt"]) + j.astype(U64) * U64(CHECKPOINT_DTYPE.itemsize) if ckpt else None
    return jobs, dst, ck, layout


def parent_arrays(objects, *, bases=BASES, sha1=True, crc32=True, ckpt=False, copy=None, fresh=True, running=False):
    """The construction of DeviceObjects.__init__ before the builder (build="host"), lifted: the loops over the
    Python lists, the field-by-field fill, default_copy_offsets with its alignment as a parameter.  It always
    passes a status pointer.  Returns jobs, dst, ckpt pointers, copy_offsets, copy_bytes."""
    objects = [list(o) for o in objects]
    nobjects = len(objects)
    counts = np.array([len(o) for o in objects], dtype=np.int64)
    n = int(counts.sum())
    first = np.concatenate(([0], np.cumsum(counts)))[:-1] if nobjects else np.zeros(0, np.int64)
    last = first + counts - 1
    ext = np.array([e for o in objects for e in o], dtype=np.uint64).reshape(n, 2)
    owner = np.repeat(np.arange(nobjects, dtype=np.uint64), counts)
    idx = np.arange(n, dtype=np.uint64)
    jobs = np.zeros(n, dtype=JOB_DTYPE)
    jobs["data"] = np.uint64(bases["data"]) + ext[:, 0]
    jobs["length"] = ext[:, 1]
    if crc32:
        jobs["crc32"] = np.uint64(bases["crc32"]) + owner * np.uint64(4)
    if sha1:
        jobs["sha1"] = np.uint64(bases["sha1"]) + owner * np.uint64(104)
    jobs["sum"] = np.uint64(bases["sums"]) + idx * np.uint64(24)
    jobs["status"] = np.uint64(bases["status"]) + idx * np.uint64(4)
    jobs["flags"] = EFES_JOB_CHAIN
    heads = first[counts > 0]
    jobs["flags"][heads] = EFES_JOB_INIT if fresh else 0
    if running:
        jobs["flags"] |= EFES_JOB_FINALIZE
    else:
        jobs["flags"][last[counts > 0]] |= EFES_JOB_FINALIZE
    ck = np.uint64(bases["ckpt"]) + idx * np.uint64(CHECKPOINT_DTYPE.itemsize) if ckpt else None
    dst = offsets = room = None
    if copy is not None:
        sizes = [sum(int(m) for _, m in o) for o in objects]
        if copy[0] == "explicit":
            offsets = np.asarray(copy[1], dtype=np.uint64)
            room = int((offsets + np.array(sizes, dtype=np.uint64)).max()) if nobjects else 0
        else:
            align = copy[1]
            offsets, at = np.zeros(len(sizes), dtype=np.uint64), 0
            for i, size in enumerate(sizes):
                at = (at + align - 1) // align * align
                offsets[i] = at
                at += size
            room = at
        before = np.cumsum(ext[:, 1]) - ext[:, 1]
        within = before - before[first[owner.astype(np.int64)]] if n else before
        dst = (np.uint64(bases["copy_to"]) + offsets[owner.astype(np.int64)] + within).astype(np.uint64)
    return jobs, dst, ck, offsets, room


class Guarded:
    """A host output array of `words` 64-bit words with GUARD sentinel words on either side, all of it pre-filled
    with the sentinel."""

    def __init__(self, words):
        self.words = words
        self.buf = np.full(words + 2 * GUARD, SENTINEL, dtype=U64)

    @property
    def ptr(self):
        return self.buf.ctypes.data + 8 * GUARD

    def body(self):
        return self.buf[GUARD:GUARD + self.words]

    def guards_intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all() and (self.buf[GUARD + self.words:] == SENTINEL).all())

    def untouched(self):
        return bool((self.buf == SENTINEL).all())


def make_table(ext, first, *, bases=BASES, sha1=True, crc32=True, status=True, ckpt=False, copy=None, flags=0,
               ext_ptr=None, first_ptr=None, offsets_ptr=None):
    """The efes_objects struct of a table; ext_ptr / first_ptr / offsets_ptr override where the three arrays lie
    (device addresses for efes_objects_jobs)."""
    explicit = copy is not None and copy[0] == "explicit"
    return Objects(data=bases["data"], extents=ext_ptr if ext_ptr is not None else (ext.ctypes.data if len(ext) else None),
                   first=first_ptr if first_ptr is not None else first.ctypes.data,
                   sha1=bases["sha1"] if sha1 else None, crc32=bases["crc32"] if crc32 else None, sums=bases["sums"],
                   status=bases["status"] if status else None, ckpt=bases["ckpt"] if ckpt else None,
                   copy_to=bases["copy_to"] if copy is not None else None,
                   copy_offsets=offsets_ptr if explicit else None, nobjects=len(first) - 1, nextents=len(ext), flags=flags,
                   copy_align=copy[1] if copy is not None and copy[0] == "default" else 0)


def run_host(efes_lib, ext, first, *, layout=True, **opts):
    """efes_objects_jobs_host over guarded outputs: (rc, jobs, dst, ckpt, layout) as Guarded arrays (None: not
    passed)."""
    import ctypes
    n, m = len(ext), len(first) - 1
    copy = opts.get("copy")
    ext = np.ascontiguousarray(ext, dtype=U64)
    first = np.ascontiguousarray(first, dtype=np.uint32)
    offs = np.ascontiguousarray(copy[1], dtype=U64) if copy is not None and copy[0] == "explicit" else None
    t = make_table(ext, first, offsets_ptr=None if offs is None else offs.ctypes.data, **opts)
    J = Guarded(7 * n)
    D = Guarded(n) if copy is not None else None
    C = Guarded(n) if opts.get("ckpt") else None
    Y = Guarded(m + 1) if layout else None
    out = ObjectsOut(jobs=J.ptr, dst=D.ptr if D else None, ckpt=C.ptr if C else None, layout=Y.ptr if Y else None)
    rc = efes_lib.lib().efes_objects_jobs_host(ctypes.byref(t), ctypes.byref(out))
    return rc, J, D, C, Y


def check_outputs(got, want, what=""):
    """got: (jobs, dst, ckpt, layout) Guarded or None; want: expectation()'s tuple.  Bodies equal, guards intact."""
    J, D, C, Y = got
    jobs, dst, ck, layout = want
    assert J.guards_intact() and (J.body() == jobs.view(U64)).all(), (what, "jobs", np.nonzero(J.body() != jobs.view(U64))[0][:8])
    if D is not None:
        assert D.guards_intact() and (D.body() == dst).all(), (what, "dst", np.nonzero(D.body() != dst)[0][:8])
    if C is not None:
        assert C.guards_intact() and (C.body() == ck).all(), (what, "ckpt")
    if Y is not None:
        assert Y.guards_intact() and (Y.body() == layout).all(), (what, "layout", Y.body()[-3:], layout[-3:])


# ---- tables
def ragged_objects(seed=7, nobjects=70, most=5, least=0, max_len=1 << 20):
    rng = random.Random(seed)
    return [[(rng.randrange(0, 1 << 30), rng.randrange(0, max_len)) for _ in range(rng.randint(least, most))]
            for _ in range(nobjects)]


def edge_tables():
    rng = random.Random(11)
    e = lambda n=None: (rng.randrange(0, 1 << 30), rng.randrange(1, 5000) if n is None else n)
    return {
        "ragged": ragged_objects(),
        "empty_first": [[], [e(), e()], [e()]],
        "empty_last": [[e()], [e(), e(), e()], []],
        "empty_runs": [[], [], [e()], [], [], [], [e(), e()], [], [e()], [], []],
        "all_empty": [[], [], []],
        "no_objects": [],
        "one_object": [[e(), e(), e(), e()]],
        "one_object_one_extent": [[e()]],
        "zero_lengths": [[e(0)], [e(), e(0), e()], [e(0), e(0)], [e(0), e()]],
        "long": [[e((1 << 32) - 1), e()], [e(1 << 32)], [e(), e((1 << 40) + 5), e(1)], [e((1 << 32) - 1), e(1 << 32), e((1 << 40) + 5)]],
    }


COPIES = [None, ("default", 1), ("default", 16), ("default", 256), ("explicit", None)]
HASHES = {"sha1": dict(sha1=True, crc32=False), "crc32": dict(sha1=False, crc32=True), "both": dict(sha1=True, crc32=True)}


def option_grid(nobjects, seed=3):
    """{FRESH or not} x {RUNNING or not} x {status NULL or not} x {ckpt or not} x the five copy modes; the explicit
    offsets are random, unaligned and unordered."""
    rng = random.Random(seed)
    for fresh, running, status, ckpt, copy in itertools.product((0, 1), (0, 1), (False, True), (False, True), COPIES):
        if copy is not None and copy[0] == "explicit":
            copy = ("explicit", np.array([rng.randrange(0, 1 << 50) for _ in range(nobjects)], dtype=U64))
        yield dict(flags=(EFES_OBJECTS_FRESH if fresh else 0) | (EFES_OBJECTS_RUNNING if running else 0), status=status,
                   ckpt=ckpt, copy=copy)


def describe(opts):
    copy = opts.get("copy")
    return {**opts, "copy": None if copy is None else copy[0] if copy[0] == "explicit" else copy}


# ---- the tests
@pytest.mark.parametrize("hashes", list(HASHES))
def test_option_grid_matches_the_contract(efes_lib, hashes):
    objects = ragged_objects()
    ext, first = table_of(objects)
    for opts in option_grid(len(objects)):
        opts.update(HASHES[hashes])
        rc, *got = run_host(efes_lib, ext, first, **opts)
        assert rc == 0, describe(opts)
        check_outputs(got, expectation(ext, first, **opts), describe(opts))


@pytest.mark.parametrize("name", list(edge_tables()))
def test_edge_tables_match_the_contract(efes_lib, name):
    objects = edge_tables()[name]
    ext, first = table_of(objects)
    for opts in option_grid(len(objects)):
        rc, *got = run_host(efes_lib, ext, first, **opts)
        assert rc == 0, (name, describe(opts))
        check_outputs(got, expectation(ext, first, **opts), (name, describe(opts)))


@pytest.mark.parametrize("name", list(edge_tables()))
@pytest.mark.parametrize("hashes", list(HASHES))
def test_matches_what_device_objects_built_on_the_host(efes_lib, name, hashes):
    """Byte for byte the arrays of the host construction (which always passes a status pointer), and its
    copy_offsets and copy_bytes in the layout."""
    objects = edge_tables()[name]
    ext, first = table_of(objects)
    for opts in option_grid(len(objects)):
        if not opts["status"]:
            continue
        opts.update(HASHES[hashes])
        rc, J, D, C, Y = run_host(efes_lib, ext, first, **opts)
        assert rc == 0
        jobs, dst, ck, offsets, room = parent_arrays(objects, sha1=opts["sha1"], crc32=opts["crc32"], ckpt=opts["ckpt"], copy=opts["copy"],
                                                     fresh=bool(opts["flags"] & EFES_OBJECTS_FRESH),
                                                     running=bool(opts["flags"] & EFES_OBJECTS_RUNNING))
        what = (name, describe(opts))
        assert J.body().tobytes() == jobs.tobytes(), what
        if opts["ckpt"]:
            assert C.body().tobytes() == ck.astype(U64).tobytes(), what
        if opts["copy"] is not None:
            assert D.body().tobytes() == dst.tobytes(), what
            assert (Y.body()[:-1] == offsets).all() and int(Y.body()[-1]) == room, what
        assert all(g is None or g.guards_intact() for g in (J, D, C, Y)), what


def test_expectation_equals_the_host_construction_on_random_tables():
    """The two references agree with each other: 100 random tables with empty objects and lengths up to 2^40."""
    rng = random.Random(2024)
    for k in range(100):
        objects = [[(rng.randrange(0, 1 << 40), rng.randrange(0, 1 << rng.choice((8, 20, 33, 40)))) for _ in range(rng.choice((0, 0, 1, 2, 5)))]
                   for _ in range(rng.randint(0, 40))]
        ext, first = table_of(objects)
        copy = rng.choice([("default", 1), ("default", 64), ("default", 256),
                           ("explicit", np.array([rng.randrange(0, 1 << 50) for _ in objects], dtype=U64))])
        fresh, running = rng.random() < 0.5, rng.random() < 0.5
        jobs, dst, ck, layout = expectation(ext, first, ckpt=True, copy=copy,
                                            flags=(EFES_OBJECTS_FRESH if fresh else 0) | (EFES_OBJECTS_RUNNING if running else 0))
        pj, pd, pc, offsets, room = parent_arrays(objects, ckpt=True, copy=copy, fresh=fresh, running=running)
        assert jobs.tobytes() == pj.tobytes() and dst.tobytes() == pd.tobytes() and ck.tobytes() == pc.astype(U64).tobytes(), k
        assert (layout[:-1] == offsets).all() and int(layout[-1]) == room, k


def test_layout_without_copy_and_outputs_not_asked_for(efes_lib):
    """layout may be asked for without copy_to (sizes and offsets only, at the default alignment); with layout
    NULL nothing but the arrays asked for is written."""
    objects = ragged_objects(seed=5)
    ext, first = table_of(objects)
    rc, *got = run_host(efes_lib, ext, first, copy=None, layout=True)
    assert rc == 0
    check_outputs(got, expectation(ext, first, copy=None))
    rc, J, D, C, Y = run_host(efes_lib, ext, first, copy=("default", 16), ckpt=True, layout=False)
    assert rc == 0 and Y is None
    check_outputs((J, D, C, None), expectation(ext, first, copy=("default", 16), ckpt=True))


def test_no_extents(efes_lib):
    """nextents == 0 writes no job; the layout is still written when asked: zeros (default) or the offsets and their
    maximum, and the single word layout[0] = 0 for no objects.  NULL extents and first are fine there."""
    import ctypes
    for m, offsets in ((0, None), (3, None), (3, [700, 90, 5000])):
        offs = None if offsets is None else np.array(offsets, dtype=U64)
        Y = Guarded(m + 1)
        t = Objects(nobjects=m, nextents=0, copy_offsets=None if offs is None else offs.ctypes.data)
        out = ObjectsOut(layout=Y.ptr)
        assert efes_lib.lib().efes_objects_jobs_host(ctypes.byref(t), ctypes.byref(out)) == 0
        want = ([0] * m if offsets is None else offsets) + [max(offsets) if offsets else 0]
        assert Y.guards_intact() and Y.body().tolist() == want, (m, offsets, Y.body())
        assert efes_lib.lib().efes_objects_jobs_host(ctypes.byref(t), ctypes.byref(ObjectsOut())) == 0
