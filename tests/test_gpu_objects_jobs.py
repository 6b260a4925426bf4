"""GPU parity of efes_objects_jobs: an object table in device memory expanded on the device into the job array,
the destination pointers, the record pointers and the gather layout.  Every case compares the device call with
the numpy expectation of test_objects_jobs_host.py and with efes_objects_jobs_host on the same table, over
outputs that carry sentinel words on either side.  The builder touches no data bytes, so the base addresses and
the lengths are fictitious except in the stream-order tests, which hash a small real set through the chain calls
with no host synchronisation between the builder and the walk.  Bit-exact."""
import ctypes
import random

import numpy as np
import pytest

from test_objects_jobs_host import (GUARD, HASHES, SENTINEL, U64, Guarded, check_outputs, describe, expectation, make_table,
                                    option_grid, parent_arrays, ragged_objects, run_host, table_of)

pytestmark = pytest.mark.gpu

BUF_BYTES = 1 << 20
TOP = 1 << 20  # EFES_OBJECTS_MAX


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from efes_amd import _lib, batch, hashing
    ctx = hashing.default_context(0)
    buf = torch.empty(BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    ctx.fill_synthetic(buf.data_ptr(), BUF_BYTES, 0x0B1EC75, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(torch=torch, hashing=hashing, batch=batch, lib=_lib, ctx=ctx, buf=buf, host=buf.cpu().numpy())


class DeviceGuarded(Guarded):
    """Guarded in device memory; fetch() brings it back for the comparisons."""

    def __init__(self, torch, words):
        self.words = words
        self.t = torch.from_numpy(np.full(words + 2 * GUARD, SENTINEL, dtype=U64).view(np.int64)).to("cuda:0")
        self.buf = None

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * GUARD

    def fetch(self):
        self.buf = self.t.cpu().numpy().view(U64)
        return self


def _up(torch, a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view)).to("cuda:0")


def run_device(env, ext, first, *, layout=True, scratch="exact", **opts):
    """efes_objects_jobs over guarded device outputs, on torch's current stream: (rc, jobs, dst, ckpt, layout)."""
    torch, L = env["torch"], env["lib"]
    n, m = len(ext), len(first) - 1
    copy = opts.get("copy")
    ext_d = _up(torch, np.asarray(ext, dtype=U64).reshape(n, 2), np.int64)
    first_d = _up(torch, np.asarray(first, dtype=np.uint32), np.int32)
    offs_d = _up(torch, np.asarray(copy[1], dtype=U64), np.int64) if copy is not None and copy[0] == "explicit" else None
    t = make_table(ext, first, ext_ptr=ext_d.data_ptr() or None, first_ptr=first_d.data_ptr(),
                   offsets_ptr=None if offs_d is None else (offs_d.data_ptr() or None), **opts)
    J = DeviceGuarded(torch, 7 * n)
    D = DeviceGuarded(torch, n) if copy is not None else None
    C = DeviceGuarded(torch, n) if opts.get("ckpt") else None
    Y = DeviceGuarded(torch, m + 1) if layout else None
    out = L.ObjectsOut(jobs=J.ptr, dst=D.ptr if D else None, ckpt=C.ptr if C else None, layout=Y.ptr if Y else None)
    need = env["hashing"].objects_jobs_scratch(m, n)
    S = torch.empty(max(need, 16) + 16, dtype=torch.uint8, device="cuda:0")
    sp, sb = {"exact": (S.data_ptr(), need), "null": (None, need), "odd": (S.data_ptr() + 8, need),
              "small": (S.data_ptr(), need - 1)}[scratch]
    torch.cuda.synchronize()  # the sentinels and the table are in place
    rc = L.lib().efes_objects_jobs(env["ctx"].handle, ctypes.byref(t), ctypes.byref(out), sp, sb,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(g.fetch() if g is not None else None for g in (J, D, C, Y))


def check_both(env, ext, first, what="", layout=True, **opts):
    """The device call against the numpy expectation and against efes_objects_jobs_host."""
    rc, *got = run_device(env, ext, first, layout=layout, **opts)
    assert rc == 0, (what, describe(opts))
    check_outputs(got, expectation(ext, first, **opts), (what, describe(opts)))
    hrc, *hgot = run_host(env["lib"], ext, first, layout=layout, **opts)
    assert hrc == 0
    for g, h in zip(got, hgot):
        assert (g is None) == (h is None) and (g is None or (g.body() == h.body()).all()), (what, describe(opts))


# ---- the scans' seams
SEAMS = sorted({1, 63, 64, 65} | {v for B in (256, 1024) for v in (B - 1, B, B + 1, 2 * B + 3)})
CROSSINGS = (31, 64, 256, 1024)  # a partial sum passes a multiple of 2^32 at this lane: inside a wavefront, at a
#                                  wavefront's first lane, at the first lane of a block of 256 and of 1024


def seam_lengths(n, rng):
    """Short lengths, with the inclusive sum brought to k 2^32 - 1 at lane c - 1 and lane c adding 2, for every
    crossing c < n: the carry out of the low 32 bits happens exactly where the scan's pieces meet."""
    lengths = [rng.randrange(0, 300) for _ in range(n)]
    for k, c in enumerate(x for x in CROSSINGS if x < n):
        lengths[c - 1] = (k + 1) * (1 << 32) - 1 - sum(lengths[:c - 1])
        lengths[c] = 2
    return lengths


def seam_table(n, m, seed):
    rng = random.Random(seed)
    ext = np.array([(rng.randrange(0, 1 << 30), x) for x in seam_lengths(n, rng)], dtype=U64).reshape(n, 2)
    if m == n:  # one extent each: the objects' sizes are the lengths, so the second scan meets the same carries
        first = np.arange(n + 1, dtype=np.uint32)
    else:
        first = np.array([0] + sorted(rng.randrange(0, n + 1) for _ in range(m - 1)) + [n], dtype=np.uint32)
    return ext, first


@pytest.mark.parametrize("nextents", SEAMS)
def test_scan_boundaries(env, nextents):
    from efes_amd._lib import OBJECTS_SCAN_BLOCK
    assert OBJECTS_SCAN_BLOCK in (256, 1024)
    rng = random.Random(nextents)
    for nobjects in SEAMS:
        ext, first = seam_table(nextents, nobjects, 1000 * nextents + nobjects)
        offsets = np.array([rng.randrange(0, 1 << 50) for _ in range(nobjects)], dtype=U64)
        for copy in (("default", 1), ("default", 256), ("explicit", offsets)):
            check_both(env, ext, first, (nextents, nobjects), ckpt=True, copy=copy, flags=1)


# ---- the limits
def _limit_table(which):
    rng = np.random.default_rng(5)
    if which == "extents":  # 2^20 extents, one object
        n, first = TOP, np.array([0, TOP], dtype=np.uint32)
    elif which == "objects":  # 2^20 objects of one extent
        n, first = TOP, np.arange(TOP + 1, dtype=np.uint32)
    else:  # 2^20 objects, all empty but the last
        n, first = 3, np.array([0] * TOP + [3], dtype=np.uint32)
    ext = np.stack([rng.integers(0, 1 << 40, n, dtype=np.uint64), rng.integers(0, 1 << 13, n, dtype=np.uint64)], axis=1)
    ext[n // 2, 1] = (1 << 40) + 5
    return ext, first


@pytest.mark.parametrize("which", ["extents", "objects", "empty_but_last"])
def test_limits(env, which):
    ext, first = _limit_table(which)
    check_both(env, ext, first, which, ckpt=True, copy=("default", 256), flags=1)
    if which != "extents":
        offsets = np.random.default_rng(6).integers(0, 1 << 50, len(first) - 1, dtype=np.uint64)
        check_both(env, ext, first, which, copy=("explicit", offsets), flags=2)


@pytest.mark.parametrize("which", ["nobjects", "nextents"])
def test_one_more_than_the_limit_is_refused(env, which):
    """EFES_ERR_ARG from the counts alone, with every output's sentinels untouched (the arrays need not have the room)."""
    torch, L = env["torch"], env["lib"]
    ext, first = table_of(ragged_objects())
    ext_d, first_d = _up(torch, ext, np.int64), _up(torch, first, np.int32)
    t = make_table(ext, first, ext_ptr=ext_d.data_ptr(), first_ptr=first_d.data_ptr(), ckpt=True, copy=("default", 256))
    setattr(t, which, TOP + 1)
    G = [DeviceGuarded(torch, 64) for _ in range(4)]
    out = L.ObjectsOut(jobs=G[0].ptr, dst=G[1].ptr, ckpt=G[2].ptr, layout=G[3].ptr)
    S = torch.empty(32 << 20, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    assert env["hashing"].objects_jobs_scratch(*((TOP + 1, 5) if which == "nobjects" else (5, TOP + 1))) == 0
    rc = L.lib().efes_objects_jobs(env["ctx"].handle, ctypes.byref(t), ctypes.byref(out), S.data_ptr(), S.numel(), None)
    torch.cuda.synchronize()
    assert rc == L.EFES_ERR_ARG and all(g.fetch().untouched() for g in G)


@pytest.mark.parametrize("scratch", ["null", "odd", "small"])
def test_scratch_errors(env, scratch):
    ext, first = table_of(ragged_objects())
    rc, *got = run_device(env, ext, first, ckpt=True, copy=("default", 256), scratch=scratch)
    assert rc == env["lib"].EFES_ERR_ARG and all(g.untouched() for g in got)


# ---- the option grid of the host test, one ragged shape
@pytest.mark.parametrize("hashes", list(HASHES))
def test_option_grid(env, hashes):
    objects = ragged_objects()  # 70 objects of 0 to 5 extents
    ext, first = table_of(objects)
    for opts in option_grid(len(objects)):
        opts.update(HASHES[hashes])
        check_both(env, ext, first, hashes, **opts)


def test_outputs_not_asked_for_are_not_needed(env):
    ext, first = table_of(ragged_objects(seed=8))
    check_both(env, ext, first, layout=False)  # jobs alone
    check_both(env, ext, first, layout=True)  # sizes and offsets without a destination
    check_both(env, ext, first, ckpt=True, layout=False)
    check_both(env, ext, first, copy=("default", 16), layout=False)


def test_no_extents(env):
    """nextents == 0 launches nothing for jobs and needs no scratch; the layout is still written."""
    none = np.zeros((0, 2), dtype=U64)
    for m, copy in ((0, None), (3, None), (1500, None), (3, ("explicit", [700, 90, 5000])),
                    (1500, ("explicit", list(range(7, 7 + 3 * 1500, 3))))):
        first = np.zeros(m + 1, dtype=np.uint32)
        rc, J, D, C, Y = run_device(env, none, first, copy=copy, scratch="null")
        assert rc == 0 and J.untouched() and Y.guards_intact()
        want = ([0] * m if copy is None else list(copy[1])) + [max(copy[1]) if copy else 0]
        assert Y.body().tolist() == want, (m, Y.body()[-4:])


# ---- a table that breaks the rules
@pytest.mark.parametrize("how", ["swap", "first0", "last_short", "last_long", "huge"])
def test_malformed_table_stays_in_range(env, how):
    """Every state pointer emitted lies inside its state array, every sum, status and record pointer is the one
    of its own j, and the guards survive; the content is otherwise not compared."""
    from test_objects_jobs_host import BASES
    ext, first = table_of(ragged_objects(seed=21))
    n, m = len(ext), len(first) - 1
    first = first.copy()
    if how == "swap":
        a, b = 10, 40
        assert first[a] != first[b]
        first[a], first[b] = first[b], first[a]
    elif how == "first0":
        first[0] = 3
    elif how == "last_short":
        first[m] = n - 4
    elif how == "last_long":
        first[m] = n + 1000
    else:
        first[m // 2] = 0xFFFFFFFF
    for copy in (("default", 256), ("explicit", np.arange(m, dtype=U64) * U64(4096))):
        rc, J, D, C, Y = run_device(env, ext, first, ckpt=True, copy=copy, flags=1)
        assert rc == 0 and all(g.guards_intact() for g in (J, D, C, Y))
        jobs = J.body().view(env["lib"].JOB_DTYPE)
        j = np.arange(n, dtype=U64)
        for field, stride in (("sha1", 104), ("crc32", 4)):
            rel = jobs[field] - U64(BASES[field])
            assert (rel % U64(stride) == 0).all() and (rel // U64(stride) < U64(m)).all(), (how, field)
        assert (jobs["sum"] == U64(BASES["sums"]) + j * U64(24)).all() and (jobs["status"] == U64(BASES["status"]) + j * U64(4)).all()
        assert (C.body() == U64(BASES["ckpt"]) + j * U64(112)).all()
        assert (jobs["data"] == U64(BASES["data"]) + ext[:, 0]).all() and (jobs["length"] == ext[:, 1]).all()
        assert (jobs["_reserved"] == 0).all() and (jobs["flags"] & ~np.uint32(0xB) == 0).all()


# ---- stream order: the builder directly in front of the walks
def real_objects():
    """70 objects of 1 to 5 extents of 0 to 300 bytes at odd offsets."""
    rng = random.Random(99)
    return [[(2 * rng.randrange(0, (BUF_BYTES - 400) // 2) + 1, rng.randrange(0, 301)) for _ in range(rng.randint(1, 5))]
            for _ in range(70)]


CALLS = {"efes_crc32_chain": dict(), "efes_crc32_copy": dict(copy=True), "efes_hash_chain": dict(sha1=True),
         "efes_hash_chain_wide": dict(sha1=True, walk="wide"),
         "efes_hash_chain_wide_copy": dict(sha1=True, walk="wide", copy=True, checkpoints=True)}


def _bases(env, O):
    return dict(data=env["buf"].data_ptr(), sha1=O.states.data_ptr() if O.has_sha1 else 0, crc32=O.crcs.data_ptr(),
                sums=O.sums.data_ptr(), status=O.status.data_ptr(), ckpt=O.ckpt.data_ptr() if O.has_checkpoints else 0,
                copy_to=O.copy_to or 0)


def _arrays(O):
    """The three arrays as they lie on the device (None: the set has none)."""
    n = O.n
    return (O.jobs.cpu().numpy()[: 56 * n].tobytes(), O._dst.cpu().numpy()[: 8 * n].tobytes() if O.copy_to is not None else None,
            O._ckpt_ptrs.cpu().numpy()[: 8 * n].tobytes() if O.has_checkpoints else None)


@pytest.mark.parametrize("stream", ["null", "side"])
@pytest.mark.parametrize("call", list(CALLS))
def test_stream_order(env, call, stream):
    """build="device" and submit() with no host synchronisation in between, against the build="host" set: statuses,
    states, sums, records and gathered bytes are the same, and the three arrays are byte for byte what the host
    construction makes for the same base addresses."""
    torch, batch = env["torch"], env["batch"]
    kw = dict(CALLS[call])
    copy = kw.pop("copy", False)
    objects = real_objects()
    room = batch.default_copy_offsets(objects)[1]
    side = torch.cuda.Stream() if stream == "side" else torch.cuda.current_stream()
    sets, landed = {}, {}
    with torch.cuda.stream(side):
        for build in ("host", "device"):
            landed[build] = torch.full((room + 512,), 0xEE, dtype=torch.uint8, device="cuda:0")
            O = batch.DeviceObjects(env["buf"].data_ptr(), objects, running=True, ctx=env["ctx"], build=build,
                                    copy_to=landed[build].data_ptr() + 256 if copy else None, **kw)
            O.submit()  # directly behind the builder
            sets[build] = O
    torch.cuda.synchronize()
    H, D = sets["host"], sets["device"]
    assert (H.status_host() == 0).all() and (D.status_host() == 0).all()
    assert (D.crc_sum() == H.crc_sum()).all() and (D.sums.cpu().numpy() == H.sums.cpu().numpy()).all()
    assert D.running_crcs().tolist() == H.running_crcs().tolist()
    if kw.get("sha1"):
        assert D.states_host().tobytes() == H.states_host().tobytes() and D.running_sha1() == H.running_sha1()
        assert D.sha1_hex() == H.sha1_hex()
    if kw.get("checkpoints"):
        assert D.checkpoints_host().tobytes() == H.checkpoints_host().tobytes()
    if copy:
        assert (landed["device"].cpu().numpy() == landed["host"].cpu().numpy()).all()
        assert (D.copy_offsets == H.copy_offsets).all() and D.copy_offsets.dtype == H.copy_offsets.dtype
        assert D.copy_bytes == H.copy_bytes == room
    for O in (H, D):  # the lifted construction is the host build's, and the device build's arrays are its bytes
        jobs, dst, ck, _, _ = parent_arrays(objects, bases=_bases(env, O), sha1=bool(kw.get("sha1")), crc32=True,
                                            ckpt=bool(kw.get("checkpoints")), copy=("default", 256) if copy else None,
                                            fresh=True, running=True)
        want = (jobs.tobytes(), dst.tobytes() if copy else None, ck.astype(U64).tobytes() if ck is not None else None)
        assert _arrays(O) == want, (call, O.build)
    assert D.jobs_host.tobytes() == _arrays(D)[0] and D.jobs_host.dtype == H.jobs_host.dtype


def test_build_device_with_options(env):
    """Not fresh, not running, seeded CRCs, explicit offsets, objects without extents: the same values as build="host"."""
    torch, batch = env["torch"], env["batch"]
    rng = random.Random(5)
    objects = [o if k % 7 else [] for k, o in enumerate(real_objects())]
    crcs = np.array([rng.randrange(0, 1 << 32) for _ in objects], dtype=np.uint32)
    offsets = np.array([2048 * k + 3 for k in range(len(objects))], dtype=np.uint64)
    got = {}
    for build in ("host", "device"):
        landed = torch.full((2048 * len(objects) + 4096,), 0xEE, dtype=torch.uint8, device="cuda:0")
        O = batch.DeviceObjects(env["buf"].data_ptr(), objects, fresh=False, crcs=crcs, ctx=env["ctx"], build=build,
                                copy_to=landed.data_ptr(), copy_offsets=offsets)
        O.run()
        got[build] = (O.status_host().tolist(), O.crc_sum().tolist(), O.sums.cpu().numpy().tobytes(), landed.cpu().numpy().tobytes(),
                      O.copy_offsets.tolist(), O.copy_bytes, O.first.tolist(), O.last.tolist())
    assert got["device"] == got["host"]


@pytest.mark.parametrize("kind", ["crc", "wide_copy_ckpt"])
def test_from_table(env, kind):
    """The set of a table that already lies in device memory gives what the list constructor gives, and does not
    fetch the table while it is built and submitted."""
    torch, batch = env["torch"], env["batch"]
    objects = [o if k % 9 else [] for k, o in enumerate(real_objects())] + [[]]
    ext, first = table_of(objects)
    kw = dict(sha1=True, walk="wide", checkpoints=True) if kind == "wide_copy_ckpt" else {}
    room = batch.default_copy_offsets(objects)[1]
    landed = [torch.full((room + 512,), 0xEE, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    H = batch.DeviceObjects(env["buf"].data_ptr(), objects, running=True, ctx=env["ctx"], copy_to=landed[0].data_ptr() + 256, **kw)
    H.run()
    T = batch.DeviceObjects.from_table(env["buf"].data_ptr(), _up(torch, ext, np.int64), _up(torch, first, np.int32), running=True,
                                       ctx=env["ctx"], copy_to=landed[1].data_ptr() + 256, **kw)
    T.submit()
    assert not {"first", "last", "copy_offsets", "copy_bytes", "jobs_host"} & set(T.__dict__)
    torch.cuda.synchronize()
    assert (T.n, T.nobjects) == (H.n, H.nobjects)
    assert T.status_host().tolist() == H.status_host().tolist() and T.crc_sum().tolist() == H.crc_sum().tolist()
    assert T.running_crcs().tolist() == H.running_crcs().tolist()
    assert (landed[1].cpu().numpy() == landed[0].cpu().numpy()).all()
    assert T.copy_offsets.tolist() == H.copy_offsets.tolist() and T.copy_bytes == H.copy_bytes
    assert T.first.tolist() == H.first.tolist() and T.last.tolist() == H.last.tolist()
    if kw:
        assert T.sha1_hex() == H.sha1_hex() and None in T.sha1_hex()
        assert T.checkpoints_host().tobytes() == H.checkpoints_host().tobytes()
        assert T.checkpoint_texts() == H.checkpoint_texts()
    with pytest.raises(ValueError, match="chain count"):
        batch.DeviceObjects.from_table(env["buf"].data_ptr(), _up(torch, ext, np.int64), _up(torch, first, np.int32), sha1=True,
                                       walk="auto_wide", ctx=env["ctx"])
