"""GPU parity of efes_objects_results: the sums and statuses a chain call leaves per extent, sorted out per object
on the device.  Every case compares the device call with the numpy expectation of test_objects_results_host.py and,
byte for byte, with efes_objects_results_host on the same inputs, over outputs that carry sentinel words on either
side.  The call touches no data, so sums and statuses are synthetic except in the stream-order tests, which hash a
small real set with no host synchronisation between the builder, the walk and the results.  Bit-exact."""
import ctypes
import hashlib
import random
import zlib

import numpy as np
import pytest

from test_objects_results_host import (GUARD, MASKS, SENTINEL, Guarded, check_outputs, expectation, make_request,
                                       make_table, own_sums, random_first, random_inputs, run_host)

pytestmark = pytest.mark.gpu

BUF_BYTES = 1 << 20
TOP = 1 << 20  # EFES_OBJECTS_MAX
SEAMS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2051]
SHA1, CRC32 = 1, 2


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

    torch = None

    def __init__(self, words):
        self.words = words
        self.t = self.torch.from_numpy(np.full(words + 2 * GUARD, SENTINEL, dtype=np.uint32).view(np.int32)).to("cuda:0")
        self.buf = None

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    def fetch(self):
        self.buf = self.t.cpu().numpy().view(np.uint32)
        return self


def _up(torch, a, view):
    return torch.from_numpy(np.ascontiguousarray(a).view(view)).to("cuda:0")


def run_device(env, first, status, sums, expected=None, compare=3, scratch="exact", spoil=None, **outs):
    """efes_objects_results over guarded device outputs, on torch's current stream: (rc, results, bad, counts)."""
    torch, L = env["torch"], env["lib"]
    DeviceGuarded.torch = torch
    m, n = len(first) - 1, len(status)
    first_d = _up(torch, np.asarray(first, dtype=np.uint32), np.int32)
    status_d = _up(torch, np.asarray(status, dtype=np.int32), np.int32)
    sums_d = _up(torch, np.asarray(sums, dtype=np.uint8).reshape(-1), np.uint8)
    exp_d = None if expected is None else _up(torch, np.asarray(expected, dtype=np.uint8).reshape(-1), np.uint8)
    t = make_table(first_d.data_ptr(), sums_d.data_ptr() or None, status_d.data_ptr() or None, m, n)
    req, R, B, C = make_request(m, expected_ptr=None if exp_d is None else (exp_d.data_ptr() or None), compare=compare,
                                guarded=DeviceGuarded, **outs)
    need = env["hashing"].objects_results_scratch(m, n)
    S = torch.empty(need + 16, dtype=torch.uint8, device="cuda:0")
    sp, sb = {"exact": (S.data_ptr(), need), "null": (None, need), "odd": (S.data_ptr() + 8, need),
              "small": (S.data_ptr(), need - 1)}[scratch]
    if spoil is not None:
        spoil(t, req)
    torch.cuda.synchronize()  # the sentinels and the inputs are in place
    rc = L.lib().efes_objects_results(env["ctx"].handle, ctypes.byref(t), ctypes.byref(req), sp, sb,
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(g.fetch() if g is not None else None for g in (R, B, C))


def check_both(env, first, status, sums, expected=None, compare=3, what="", **outs):
    """The device call against the numpy expectation and against efes_objects_results_host."""
    rc, *got = run_device(env, first, status, sums, expected, compare, **outs)
    assert rc == 0, what
    check_outputs(got, expectation(first, status, sums, expected, compare), what)
    hrc, *hgot = run_host(env["lib"], first, status, sums, expected, compare, **outs)
    assert hrc == 0
    for g, h in zip(got, hgot):
        assert (g is None) == (h is None) and (g is None or g.body().tobytes() == h.body().tobytes()), what
    return got


# ---- the scan's seams
def seam_first(m, n, rng):
    """With n >= m every object has extents (distinct cuts), so any object can be made bad; else some are empty."""
    if n < m:
        return random_first(m, n, rng)
    cuts = np.sort(rng.choice(np.arange(1, n), m - 1, replace=False)) if m > 1 else np.zeros(0, np.int64)
    return np.concatenate(([0], cuts, [n])).astype(np.uint32)


PLACEMENTS = {"all": lambda i, m: np.ones(m, bool), "none": lambda i, m: np.zeros(m, bool), "last": lambda i, m: i == m - 1,
              "every_64th": lambda i, m: i % 64 == 0, "every_1024th_plus_one": lambda i, m: i % 1024 == 1}


def plant(first, chosen, rng):
    """Statuses, sums and expected digests for which exactly the chosen objects that have extents are bad: they
    alternate between a digest that differs in one byte and a member that failed."""
    m, n = len(first) - 1, int(first[-1])
    status, sums = random_inputs(n, rng, statuses=False)
    has = first[1:] > first[:-1]
    planted = np.nonzero(chosen & has)[0]
    for k, i in enumerate(planted):
        if k % 2:
            status[rng.integers(int(first[i]), int(first[i + 1]))] = (-2, -4, -99)[k % 3]
    exp = own_sums(first, status, sums)
    spoil = planted[::2]
    exp[spoil, rng.integers(0, 24, len(spoil))] ^= 0x01
    return status, sums, exp, planted


@pytest.mark.parametrize("nobjects", SEAMS)
def test_parity_at_the_seams(env, nobjects):
    rng = np.random.default_rng(nobjects)
    i = np.arange(nobjects)
    for n in SEAMS:
        first = seam_first(nobjects, n, rng)
        for name, place in PLACEMENTS.items():
            status, sums, exp, planted = plant(first, place(i, nobjects), rng)
            R, B, C = check_both(env, first, status, sums, exp, 3, (nobjects, n, name))
            assert B.body()[:len(planted)].tolist() == planted.tolist(), (nobjects, n, name)
        status, sums = random_inputs(n, rng)  # members failing anywhere, and no list asked for
        check_both(env, first, status, sums, own_sums(first, status, sums), 3, (nobjects, n, "random"))
        check_both(env, first, status, sums, None, 0, (nobjects, n, "counts only"), results=False, bad=False)


# ---- the limits: also the cases in which a per-object loop over members would not finish in seconds
@pytest.fixture(scope="module")
def top_sums():
    return np.random.default_rng(5).integers(0, 256, (TOP, 24), dtype=np.uint8)


@pytest.mark.parametrize("at", [0, TOP // 2, TOP - 1])
def test_limit_one_object_owns_every_extent(env, top_sums, at):
    first = np.array([0, TOP], dtype=np.uint32)
    status = np.zeros(TOP, np.int32)
    status[at] = -2
    R, B, C = check_both(env, first, status, top_sums, top_sums[-1:], 3, at)
    assert C.body().tolist() == [0, 0, 1, 0] and B.body()[0] == 0
    assert R.body().view(env["lib"].OBJECT_RESULT_DTYPE)["status"][0] == -2


def test_limit_one_extent_each(env, top_sums):
    rng = np.random.default_rng(9)
    first = np.arange(TOP + 1, dtype=np.uint32)
    status = np.zeros(TOP, np.int32)
    bad = rng.random(TOP) < 0.01
    failed = bad & (rng.random(TOP) < 0.5)
    status[failed] = -4
    exp = top_sums.copy()
    exp[bad & ~failed, 20] ^= 0x80
    R, B, C = check_both(env, first, status, top_sums, exp, 3, "objects")
    assert C.body().tolist() == [TOP - int(bad.sum()), int((bad & ~failed).sum()), int(failed.sum()), 0]
    assert (B.body()[:int(bad.sum())] == np.nonzero(bad)[0]).all()


def test_limit_all_empty_but_the_last(env, top_sums):
    first = np.array([0] * TOP + [3], dtype=np.uint32)
    status = np.array([0, -99, 0], np.int32)
    R, B, C = check_both(env, first, status, top_sums[:3], None, 3, "empty_but_last")
    assert C.body().tolist() == [0, 0, 1, TOP - 1] and B.body()[0] == TOP - 1
    status[1] = 0
    exp = np.zeros((TOP, 24), np.uint8)
    exp[-1] = top_sums[2]
    R, B, C = check_both(env, first, status, top_sums[:3], exp, 3, "empty_but_last, whole")
    assert C.body().tolist() == [1, 0, 0, TOP - 1]


# ---- arguments
@pytest.mark.parametrize("scratch", ["null", "odd", "small"])
def test_scratch_errors(env, scratch):
    rng = np.random.default_rng(2)
    first = random_first(70, 200, rng)
    status, sums = random_inputs(200, rng)
    rc, *got = run_device(env, first, status, sums, own_sums(first, status, sums), 3, scratch=scratch)
    assert rc == env["lib"].EFES_ERR_ARG and all(g.untouched() for g in got)


def _set(where, field, value):
    def spoil(t, req):
        o = t if where == "table" else req
        setattr(o, field, value if not callable(value) else value(getattr(o, field)))
    return spoil


SPOILED = {"compare": _set("req", "compare", 4), "reserved": _set("req", "_reserved", 1), "counts_null": _set("req", "counts", None),
           "results_misaligned": _set("req", "results", lambda p: p + 4), "bad_misaligned": _set("req", "bad", lambda p: p + 2),
           "expected_misaligned": _set("req", "expected", lambda p: p + 2), "sums_misaligned": _set("table", "sums", lambda p: p + 1),
           "status_null": _set("table", "status", None), "first_null": _set("table", "first", None),
           "nextents": _set("table", "nextents", TOP + 1)}


@pytest.mark.parametrize("what", list(SPOILED))
def test_device_call_applies_the_shared_checks(env, what):
    """With a real context, a good scratch and guarded outputs: the device call refuses what results_check refuses,
    and writes nothing."""
    rng = np.random.default_rng(6)
    first = random_first(70, 200, rng)
    status, sums = random_inputs(200, rng)
    rc, *got = run_device(env, first, status, sums, own_sums(first, status, sums), 3, spoil=SPOILED[what])
    assert rc == env["lib"].EFES_ERR_ARG and all(g.untouched() for g in got), what


def test_no_objects(env):
    """nobjects == 0: the four counters are zero and nothing else is written; no scratch is needed."""
    rng = np.random.default_rng(4)
    for n in (0, 5, 1025):
        status, sums = random_inputs(n, rng)
        rc, R, B, C = run_device(env, np.array([0], np.uint32), status, sums, None, 3, scratch="null")
        assert rc == 0 and C.guards_intact() and C.body().tolist() == [0, 0, 0, 0]
        assert R.untouched() and B.untouched()


def test_invalid_tables_stay_in_range(env):
    """EFES_OK and intact guards for tables that break the rules, and the host twin's bytes: both sides apply the
    same clamps."""
    from test_objects_results_host import invalid_tables
    rng = np.random.default_rng(1)
    status, sums = random_inputs(90, rng)
    for name, first in invalid_tables().items():
        exp = rng.integers(0, 256, (len(first) - 1, 24), dtype=np.uint8)
        rc, *got = run_device(env, first, status, sums, exp, 3)
        assert rc == 0 and all(g.guards_intact() for g in got), name
        hrc, *hgot = run_host(env["lib"], first, status, sums, exp, 3)
        assert hrc == 0 and all(g.body().tobytes() == h.body().tobytes() for g, h in zip(got, hgot)), name


# ---- stream order, real bytes
def real_objects(seed=99, count=300):
    """About 300 objects of 0 to 5 extents of 0 to 700 bytes at odd offsets."""
    rng = random.Random(seed)
    return [[(2 * rng.randrange(0, (BUF_BYTES - 800) // 2) + 1, rng.randrange(0, 701)) for _ in range(rng.randint(0, 5))]
            for _ in range(count)]


def digests_of(host, objects):
    """(nobjects, 24): hashlib's SHA-1 and zlib's CRC-32 (big-endian) of every object's bytes; zeros without extents."""
    out = np.zeros((len(objects), 24), np.uint8)
    for i, obj in enumerate(objects):
        if obj:
            data = b"".join(host[o:o + n].tobytes() for o, n in obj)
            out[i] = np.frombuffer(hashlib.sha1(data).digest() + zlib.crc32(data).to_bytes(4, "big"), np.uint8)
    return out


def corrupt(true, objects, seed=3):
    """A tenth of the digests of objects with extents corrupted: alternately in the SHA-1 part and in the CRC only.
    Returns the expected array and the corrupted indices of either kind."""
    rng = random.Random(seed)
    exp = true.copy()
    some = sorted(rng.sample([i for i, o in enumerate(objects) if o], len(objects) // 10))
    in_sha, in_crc = some[0::2], some[1::2]
    for i in in_sha:
        exp[i, rng.randrange(0, 20)] ^= 0x10
    for i in in_crc:
        exp[i, rng.randrange(20, 24)] ^= 0x10
    return exp, in_sha, in_crc


@pytest.mark.parametrize("call", ["efes_hash_chain_wide", "efes_crc32_chain"])
def test_stream_order(env, call):
    """efes_objects_jobs -> the walk -> efes_objects_results on one stream with no host synchronisation in between;
    verdicts, bad and counts are exactly the planted ones under each mask."""
    torch, L, batch = env["torch"], env["lib"], env["batch"]
    DeviceGuarded.torch = torch
    objects = real_objects()
    m = len(objects)
    true = digests_of(env["host"], objects)
    exp, in_sha, in_crc = corrupt(true, objects)
    empty = [i for i, o in enumerate(objects) if not o]
    assert empty and in_sha and in_crc
    wide = call == "efes_hash_chain_wide"
    masks = MASKS if wide else [CRC32]
    # everything the results call needs is on the device before the first of the three calls is queued
    exp_d = _up(torch, exp.reshape(-1), np.uint8)
    outs = [make_request(m, expected_ptr=exp_d.data_ptr(), compare=c, guarded=DeviceGuarded) for c in masks]
    S = torch.empty(env["hashing"].objects_results_scratch(m, sum(len(o) for o in objects)), dtype=torch.uint8, device="cuda:0")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        O = batch.DeviceObjects(env["buf"].data_ptr(), objects, ctx=env["ctx"], build="device",
                                **(dict(sha1=True, walk="wide") if wide else {}))  # efes_objects_jobs, queued
        O.submit()  # the walk, directly behind it
        t = make_table(O._table_first.data_ptr(), O.sums.data_ptr(), O.status.data_ptr(), m, O.n)
        for req, R, B, C in outs:
            assert L.lib().efes_objects_results(env["ctx"].handle, ctypes.byref(t), ctypes.byref(req), S.data_ptr(), S.numel(),
                                                side.cuda_stream) == 0
    torch.cuda.synchronize()
    assert (O.status_host() == 0).all()
    for compare, (req, R, B, C) in zip(masks, outs):
        R.fetch(), B.fetch(), C.fetch()
        bad = sorted((in_sha if compare & SHA1 else []) + (in_crc if compare & CRC32 else []))
        rec = R.body().view(L.OBJECT_RESULT_DTYPE)
        assert R.guards_intact() and B.guards_intact() and C.guards_intact()
        assert C.body().tolist() == [m - len(empty) - len(bad), len(bad), 0, len(empty)], (call, compare)
        assert B.body()[:len(bad)].tolist() == bad and (B.body()[len(bad):] == SENTINEL).all(), (call, compare)
        want = np.zeros(m, np.uint32)
        want[empty], want[bad] = L.EFES_VERDICT_EMPTY, L.EFES_VERDICT_MISMATCH
        assert (rec["verdict"] == want).all() and (rec["status"] == 0).all(), (call, compare)
        assert (rec["sum"][:, 20:] == true[:, 20:]).all()  # hashlib and zlib, not this library
        if wide:
            assert (rec["sum"] == true).all()


def test_a_failing_member(env):
    """A middle member made invalid on the device, behind the builder: its object comes out FAILED with status
    EFES_ERR_ARG and a zero sum (the members behind an invalid one are invalid too), its neighbours unaffected."""
    torch, L, batch = env["torch"], env["lib"], env["batch"]
    objects = real_objects(seed=5, count=40)
    victim = next(i for i, o in enumerate(objects) if len(o) >= 3 and 0 < i < len(objects) - 1)
    true = digests_of(env["host"], objects)
    O = batch.DeviceObjects(env["buf"].data_ptr(), objects, ctx=env["ctx"], build="device", sha1=True, walk="wide")
    j = sum(len(o) for o in objects[:victim]) + 1
    flags = torch.tensor([L.EFES_JOB_CHAIN | L.EFES_JOB_INIT, 0, 0, 0], dtype=torch.uint8, device="cuda:0")
    O.jobs[56 * j + 48:56 * j + 52] = flags  # in stream order behind efes_objects_jobs
    O.submit()
    rec, counts, bad = O.results(true)
    empty = sum(1 for o in objects if not o)
    assert bad.tolist() == [victim] and counts.tolist() == [len(objects) - empty - 1, 0, 1, empty]
    assert rec["verdict"][victim] == L.EFES_VERDICT_FAILED and rec["status"][victim] == L.EFES_ERR_ARG
    assert (rec["sum"][victim] == 0).all()
    others = np.arange(len(objects)) != victim
    assert (rec["sum"][others] == true[others]).all() and (rec["status"][others] == 0).all()
    status = O.status_host()
    assert status[j] == L.EFES_ERR_ARG and (status[:j] == 0).all()


# ---- the Python layer
@pytest.mark.parametrize("build", ["host", "device", "from_table"])
@pytest.mark.parametrize("kind", ["fused", "crc"])
def test_device_objects_verify_and_results(env, build, kind):
    torch, L, batch = env["torch"], env["lib"], env["batch"]
    objects = real_objects(seed=12, count=120)
    kw = dict(sha1=True, walk="wide") if kind == "fused" else {}
    if build == "from_table":
        from test_objects_jobs_host import table_of
        ext, first = table_of(objects)
        O = batch.DeviceObjects.from_table(env["buf"].data_ptr(), _up(torch, ext, np.int64), _up(torch, first, np.int32),
                                           ctx=env["ctx"], **kw)
    else:
        O = batch.DeviceObjects(env["buf"].data_ptr(), objects, ctx=env["ctx"], build=build, **kw)
    O.submit()
    true = digests_of(env["host"], objects)
    exp, in_sha, in_crc = corrupt(true, objects, seed=8)
    planted = sorted(in_sha + in_crc) if kind == "fused" else sorted(in_crc)  # the default mask: what the set keeps
    empty = [i for i, o in enumerate(objects) if not o]
    counts, bad = O.verify(exp)
    if build == "from_table":
        assert not {"first", "last"} & set(O.__dict__), "verify() fetched the table"
    want_counts = [len(objects) - len(empty) - len(planted), len(planted), 0, len(empty)]
    assert bad.tolist() == planted and counts.tolist() == want_counts and bad.dtype == counts.dtype == np.uint32
    assert O.verify(exp, CRC32)[1].tolist() == sorted(in_crc)
    assert O.verify(_up(torch, exp, np.uint8).reshape(len(objects), 24))[1].tolist() == planted  # a device tensor
    assert O.verify(None)[0].tolist() == [len(objects) - len(empty), 0, 0, len(empty)]
    rec, counts, bad = O.results(exp)
    assert rec.dtype == L.OBJECT_RESULT_DTYPE and rec.shape == (len(objects),)
    assert bad.tolist() == planted and counts.tolist() == want_counts
    # the existing result methods of the same set
    assert (O.status_host() == 0).all() and (rec["status"] == 0).all()
    crc = rec["sum"][:, 20:].copy().view(">u4").reshape(-1)
    has = np.array([bool(o) for o in objects])
    assert (crc[has] == O.crc_sum()[has]).all() and (rec["sum"][~has] == 0).all()
    assert (rec["verdict"][~has] == L.EFES_VERDICT_EMPTY).all()
    if kind == "fused":
        assert [bytes(r[:20]).hex() if h else None for r, h in zip(rec["sum"], has)] == O.sha1_hex()
    # a second run gives the same answer
    O.reset()
    O.run()
    again = O.results(exp)
    assert again[0].tobytes() == rec.tobytes() and again[1].tolist() == want_counts and again[2].tolist() == planted
    assert O.verify(exp)[1].tolist() == planted
