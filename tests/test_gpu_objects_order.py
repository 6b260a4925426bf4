"""GPU parity of efes_objects_order and efes_objects_jobs_ordered: the longest-first ranking of an object table,
sorted on the device, and the job array emitted in that (or any) order.  Every case compares the device call with
its host twin and with the numpy reference of test_objects_order_host.py, bit for bit, over outputs that carry
sentinel words on either side.  Neither call touches data bytes, so base addresses and lengths are fictitious
except in the end-to-end and stream-order tests, which hash a small real set through every chain call and compare
what the walks leave with the same set in table order."""
import ctypes
import random

import numpy as np
import pytest

from test_objects_jobs_host import HASHES, U64, describe, make_table, option_grid, ragged_objects, table_of
from test_objects_order_host import (GUARD32, SENTINEL32, TOP, Guarded32, check_in_range, check_ordered, lengths_table,
                                     one_byte_lengths, ordered_expectation, reference_order, run_order_host, run_ordered_host)
from test_gpu_objects_jobs import DeviceGuarded, _up, run_device

pytestmark = pytest.mark.gpu

BUF_BYTES = 1 << 20


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
    return dict(torch=torch, hashing=hashing, batch=batch, lib=_lib, ctx=ctx, buf=buf)


class DeviceGuarded32(Guarded32):
    """Guarded32 in device memory; fetch() brings it back for the comparisons."""

    def __init__(self, torch, words):
        self.words = words
        self.t = torch.from_numpy(np.full(words + 2 * GUARD32, SENTINEL32, dtype=np.uint32).view(np.int32)).to("cuda:0")
        self.buf = None

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD32

    def fetch(self):
        self.buf = self.t.cpu().numpy().view(np.uint32)
        return self


def _scratch(torch, need, how):
    S = torch.empty(max(need, 16) + 16, dtype=torch.uint8, device="cuda:0")
    return S, {"exact": (S.data_ptr(), need), "null": (None, need), "odd": (S.data_ptr() + 8, need), "small": (S.data_ptr(), need - 1)}[how]


def run_order_device(env, ext, first, scratch="exact"):
    """efes_objects_order over a guarded device output, on torch's current stream: (rc, order)."""
    torch, L = env["torch"], env["lib"]
    n, m = len(ext), len(first) - 1
    ext_d = _up(torch, np.asarray(ext, dtype=U64).reshape(n, 2), np.int64)
    first_d = _up(torch, np.asarray(first, dtype=np.uint32), np.int32)
    t = L.Objects(extents=ext_d.data_ptr() or None, first=first_d.data_ptr(), nobjects=m, nextents=n)
    G = DeviceGuarded32(torch, m)
    S, (sp, sb) = _scratch(torch, env["hashing"].objects_order_scratch(m, n), scratch)
    torch.cuda.synchronize()
    rc = L.lib().efes_objects_order(env["ctx"].handle, ctypes.byref(t), G.ptr, sp, sb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, G.fetch()


def check_order(env, ext, first, what=""):
    """The device call against the host twin and against numpy."""
    rc, G = run_order_device(env, ext, first)
    hrc, H = run_order_host(env["lib"], ext, first)
    assert rc == 0 and hrc == 0 and G.guards_intact(), what
    want = reference_order(ext, first)
    bad = np.nonzero(G.body() != want)[0]
    assert bad.size == 0, (what, bad[:8], G.body()[bad[:8]], want[bad[:8]])
    assert (H.body() == want).all(), what


def run_ordered_device(env, ext, first, order, *, layout=True, job_first=True, scratch="exact", **opts):
    """efes_objects_jobs_ordered over guarded device outputs: (rc, jobs, dst, ckpt, layout, job_first)."""
    torch, L = env["torch"], env["lib"]
    n, m = len(ext), len(first) - 1
    copy = opts.get("copy")
    ext_d = _up(torch, np.asarray(ext, dtype=U64).reshape(n, 2), np.int64)
    first_d = _up(torch, np.asarray(first, dtype=np.uint32), np.int32)
    order_d = _up(torch, np.asarray(order, dtype=np.uint32), np.int32)
    offs_d = _up(torch, np.asarray(copy[1], dtype=U64), np.int64) if copy is not None and copy[0] == "explicit" else None
    t = make_table(ext, first, ext_ptr=ext_d.data_ptr() or None, first_ptr=first_d.data_ptr(),
                   offsets_ptr=None if offs_d is None else (offs_d.data_ptr() or None), **opts)
    J = DeviceGuarded(torch, 7 * n)
    D = DeviceGuarded(torch, n) if copy is not None else None
    C = DeviceGuarded(torch, n) if opts.get("ckpt") else None
    Y = DeviceGuarded(torch, m + 1) if layout else None
    F = DeviceGuarded32(torch, m + 1) if job_first else None
    out = L.ObjectsOut(jobs=J.ptr, dst=D.ptr if D else None, ckpt=C.ptr if C else None, layout=Y.ptr if Y else None)
    S, (sp, sb) = _scratch(torch, env["hashing"].objects_jobs_ordered_scratch(m, n), scratch)
    torch.cuda.synchronize()
    rc = L.lib().efes_objects_jobs_ordered(env["ctx"].handle, ctypes.byref(t), ctypes.byref(out), order_d.data_ptr() or None,
                                           F.ptr if F else None, sp, sb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(g.fetch() if g is not None else None for g in (J, D, C, Y, F))


def check_ordered_both(env, ext, first, order, what="", well_formed=True, **opts):
    """The device call against its host twin and, for a well-formed table and a permutation, the numpy reference."""
    rc, *got = run_ordered_device(env, ext, first, order, **opts)
    hrc, *hgot = run_ordered_host(env["lib"], ext, first, order, **opts)
    assert rc == 0 and hrc == 0, (what, describe(opts))
    for g, h in zip(got, hgot):
        assert (g is None) == (h is None) and (g is None or (g.guards_intact() and (g.body() == h.body()).all())), (what, describe(opts))
    if well_formed:
        check_ordered(got, ordered_expectation(ext, first, order, **{k: v for k, v in opts.items() if k not in ("layout", "job_first")}),
                      (what, describe(opts)))
    return got


# ---- the sort: the seams of its tile and of the scan block
SEAMS = sorted({1, 2, 63, 64, 65} | {v for T in (256, 1024, 2048, 4096) for v in (T - 1, T, T + 1, 2 * T + 3)})


def ragged_small(m, seed):
    """m objects of 0 to 3 extents whose sizes stay below 2^20: real sizes, most digit passes skipped."""
    rng = random.Random(seed)
    return table_of([[(rng.randrange(0, 1 << 30), rng.randrange(0, 1 << 18)) for _ in range(rng.randint(0, 3))] for _ in range(m)])


@pytest.mark.parametrize("m", SEAMS)
def test_sort_seams(env, m):
    from efes_amd._lib import OBJECTS_ORDER_TILE, OBJECTS_SCAN_BLOCK
    assert OBJECTS_ORDER_TILE in (256, 1024, 2048, 4096) and OBJECTS_SCAN_BLOCK in (256, 1024)
    rng = np.random.default_rng(m)
    check_order(env, *lengths_table(rng.integers(0, 1 << 64, m, dtype=np.uint64, endpoint=False)), (m, "random 64-bit"))
    check_order(env, *ragged_small(m, m), (m, "sizes below 2^20"))
    check_order(env, *lengths_table(rng.integers(0, 1 << 20, m, dtype=np.uint64)), (m, "lengths below 2^20"))
    check_order(env, *lengths_table([12345] * m), (m, "all keys equal"))
    for byte in {m % 8, (m + 3) % 8}:
        check_order(env, *lengths_table(one_byte_lengths(m, byte, m + byte)), (m, "one byte differs", byte))


@pytest.mark.parametrize("byte", range(8))
def test_keys_that_differ_in_one_byte(env, byte):
    check_order(env, *lengths_table(one_byte_lengths(3000, byte, byte)), byte)


def test_heavy_ties_prove_stability(env):
    rng = np.random.default_rng(12)
    sizes = rng.choice(np.array([0, 1, 255, 256, 65536, 1 << 24, (1 << 32) + 1, 77], dtype=np.uint64), 5000)
    ext, first = lengths_table(sizes)
    check_order(env, ext, first, "ties")
    rc, G = run_order_device(env, ext, first)
    for v in np.unique(sizes):
        run = G.body()[sizes[G.body()] == v]
        assert (np.diff(run.astype(np.int64)) > 0).all(), v


def test_wrapping_sums_empty_objects_and_sorted_tables(env):
    from test_objects_order_host import order_tables
    for name, (ext, first) in order_tables().items():
        if not name.startswith(("byte", "random")):
            check_order(env, ext, first, name)


def test_the_limit(env):
    """2^20 objects of one extent each: every tile and every block of the counts' scan, once."""
    rng = np.random.default_rng(5)
    lengths = rng.integers(0, 1 << 34, TOP, dtype=np.uint64)
    lengths[rng.integers(0, TOP, 50)] = rng.integers(0, 1 << 64, 50, dtype=np.uint64, endpoint=False)
    ext = np.stack([rng.integers(0, 1 << 40, TOP, dtype=np.uint64), lengths], axis=1)
    first = np.arange(TOP + 1, dtype=np.uint32)
    rc, G = run_order_device(env, ext, first)
    assert rc == 0 and G.guards_intact()
    assert (G.body() == reference_order(ext, first)).all()


@pytest.mark.parametrize("how", ["swap", "first0", "last_short", "last_long", "huge", "random", "decreasing"])
def test_a_malformed_table_still_gives_a_permutation(env, how):
    from test_objects_order_host import malformed
    ext, first = table_of(ragged_objects(seed=21, nobjects=1500))
    first = malformed(first, len(ext), how)
    rc, G = run_order_device(env, ext, first)
    assert rc == 0 and G.guards_intact()
    assert (np.sort(G.body()) == np.arange(len(first) - 1)).all()
    assert (G.body() == run_order_host(env["lib"], ext, first)[1].body()).all()


def test_no_objects_and_no_extents(env):
    rc, G = run_order_device(env, np.zeros((0, 2), U64), np.zeros(1, np.uint32), scratch="null")
    assert rc == 0 and G.untouched()
    rc, G = run_order_device(env, np.zeros((0, 2), U64), np.zeros(1301, np.uint32))
    assert rc == 0 and G.guards_intact() and (G.body() == np.arange(1300)).all()


@pytest.mark.parametrize("scratch", ["null", "odd", "small"])
def test_scratch_errors(env, scratch):
    """EFES_ERR_ARG, and nothing is launched: every output keeps its sentinels."""
    ext, first = table_of(ragged_objects())
    rc, G = run_order_device(env, ext, first, scratch=scratch)
    assert rc == env["lib"].EFES_ERR_ARG and G.untouched()
    order = reference_order(ext, first)
    rc, *got = run_ordered_device(env, ext, first, order, ckpt=True, copy=("default", 256), scratch=scratch)
    assert rc == env["lib"].EFES_ERR_ARG and all(g.untouched() for g in got)


# ---- the ordered builder
def seam_table(n, m, seed):
    rng = random.Random(seed)
    ext = np.array([(rng.randrange(0, 1 << 30), rng.randrange(0, 1 << 40)) for _ in range(n)], dtype=U64).reshape(n, 2)
    first = np.arange(n + 1, dtype=np.uint32) if m == n else np.array([0] + sorted(rng.randrange(0, n + 1) for _ in range(m - 1)) + [n], dtype=np.uint32)
    return ext, first


@pytest.mark.parametrize("nextents", SEAMS)
def test_ordered_seams(env, nextents):
    rng = np.random.default_rng(nextents)
    for nobjects in (1, 65, 1023, 1025, 2051, nextents):
        ext, first = seam_table(nextents, nobjects, 1000 * nextents + nobjects)
        offsets = rng.integers(0, 1 << 50, nobjects, dtype=np.uint64)
        for order in (reference_order(ext, first), rng.permutation(nobjects).astype(np.uint32)):
            for copy in (("default", 256), ("explicit", offsets)):
                check_ordered_both(env, ext, first, order, (nextents, nobjects), ckpt=True, copy=copy, flags=1)


@pytest.mark.parametrize("hashes", list(HASHES))
def test_ordered_option_grid(env, hashes):
    """The option grid of the builder's tests: a permutation against the host twin and numpy, and the identity
    against efes_objects_jobs itself, byte for byte."""
    objects = ragged_objects()
    ext, first = table_of(objects)
    m = len(objects)
    order, ident = reference_order(ext, first), np.arange(m, dtype=np.uint32)
    for opts in option_grid(m):
        opts.update(HASHES[hashes])
        check_ordered_both(env, ext, first, order, hashes, **opts)
        got = check_ordered_both(env, ext, first, ident, hashes, **opts)
        rc, *built = run_device(env, ext, first, **opts)
        assert rc == 0
        for g, b in zip(got[:4], built):
            assert (g is None) == (b is None) and (g is None or g.body().tobytes() == b.body().tobytes()), describe(opts)
        assert (got[4].body() == first).all()


def test_ordered_limit(env):
    ext, first = seam_table(TOP, TOP, 5)
    ext[:, 1] &= U64((1 << 30) - 1)
    order = reference_order(ext, first)
    check_ordered_both(env, ext, first, order, "limit", ckpt=True, copy=("default", 256), flags=1)


def test_ordered_without_extents_and_outputs_not_asked_for(env):
    none = np.zeros((0, 2), dtype=U64)
    for m in (0, 3, 1500):
        order = np.arange(m, dtype=np.uint32)[::-1].copy()
        rc, J, D, C, Y, F = run_ordered_device(env, none, np.zeros(m + 1, np.uint32), order, scratch="null")
        assert rc == 0 and J.untouched() and Y.guards_intact() and F.guards_intact() and not Y.body().any() and not F.body().any()
    ext, first = table_of(ragged_objects(seed=8))
    order = reference_order(ext, first)
    check_ordered_both(env, ext, first, order, layout=False, job_first=False)
    check_ordered_both(env, ext, first, order, copy=("default", 16), ckpt=True, layout=False)


@pytest.mark.parametrize("how", ["constant", "out_of_range", "random", "duplicates", "malformed_table"])
def test_what_is_no_permutation_gives_in_range_jobs(env, how):
    """Every emitted address is checked against its array; such jobs are not run.  The device equals the host twin."""
    from test_objects_order_host import malformed
    ext, first = table_of(ragged_objects(seed=22, nobjects=1300))
    n, m = len(ext), len(first) - 1
    rng = np.random.default_rng(8)
    order = {"constant": np.full(m, int(np.argmax(np.diff(first.astype(np.int64)))), np.uint32),
             "out_of_range": np.full(m, 0xFFFFFFFF, np.uint32),
             "random": rng.integers(0, 1 << 32, m, dtype=np.uint32),
             "duplicates": rng.integers(0, m, m, dtype=np.uint32),
             "malformed_table": rng.permutation(m).astype(np.uint32)}[how]
    tables = [malformed(first, n, h) for h in ("swap", "last_short", "huge", "random")] if how == "malformed_table" else [first]
    for f in tables:
        J, D, C, Y, F = check_ordered_both(env, ext, f, order, how, well_formed=False, ckpt=True, copy=("default", 256), flags=1)
        assert Y.guards_intact()
        check_in_range(ext, m, J, D, C, F)


# ---- end to end: a small real set through every walk, in three orders
def real_objects():
    """200 shuffled objects of 0 to 5 extents of 0 to 700 bytes at odd offsets."""
    rng = random.Random(99)
    objects = [[(2 * rng.randrange(0, (BUF_BYTES - 800) // 2) + 1, rng.randrange(0, 701)) for _ in range(rng.randint(0, 5))]
               for _ in range(200)]
    rng.shuffle(objects)
    return objects


def walks(env):
    G4 = env["lib"].MODE_GROUP[4]
    return {"efes_hash_chain_wide": dict(sha1=True, walk="wide"), "EFES_MODE_GROUP4": dict(sha1=True, walk=G4),
            "efes_hash_chain": dict(sha1=True), "efes_crc32_chain": dict(), "efes_crc32_copy": dict(copy=True),
            "efes_hash_chain_wide_copy": dict(sha1=True, walk="wide", copy=True, checkpoints=True)}


WALKS = ["efes_hash_chain_wide", "EFES_MODE_GROUP4", "efes_hash_chain", "efes_crc32_chain", "efes_crc32_copy", "efes_hash_chain_wide_copy"]


def _left(O, landed):
    """Everything the walk and efes_objects_results leave, as bytes and lists."""
    rec, counts, bad = O.results()
    d = dict(status=O.status_host().tolist(), crcs=O.crc_sum().tolist(), sums=O.sums.cpu().numpy().tobytes(), records=rec.tobytes(),
             counts=counts.tolist(), bad=bad.tolist())
    if O.has_sha1:
        d["states"] = O.states_host().tobytes()
        d["sha1"] = O.sha1_hex()
    if O.has_checkpoints:
        d["ckpt"] = O.checkpoints_host().tobytes()
        d["texts"] = O.checkpoint_texts()
    if landed is not None:
        d["landed"] = landed.cpu().numpy().tobytes()
        d["layout"] = (O.copy_offsets.tolist(), O.copy_bytes)
    return d, rec


@pytest.mark.parametrize("order", ["longest_first", "permutation"])
@pytest.mark.parametrize("call", WALKS)
def test_end_to_end(env, call, order):
    torch, batch = env["torch"], env["batch"]
    kw = dict(walks(env)[call])
    copy = kw.pop("copy", False)
    objects = real_objects()
    ext, first = table_of(objects)
    m = len(objects)
    room = batch.default_copy_offsets(objects)[1]
    perm = np.random.default_rng(4).permutation(m).astype(np.uint32)
    left, sets = {}, {}
    for how in ("table", order):
        landed = torch.full((room + 512,), 0xEE, dtype=torch.uint8, device="cuda:0") if copy else None
        arg = how if how != "permutation" else _up(torch, perm, np.int32)
        O = batch.DeviceObjects(env["buf"].data_ptr(), objects, ctx=env["ctx"], build="device", order=arg,
                                copy_to=landed.data_ptr() + 256 if copy else None, **kw)
        O.run()
        left[how], rec = _left(O, landed)
        expected = np.ascontiguousarray(rec["sum"]).copy()  # what the set itself computed, two digests spoiled
        expected[3, 21] ^= 1
        expected[150, 0 if O.has_sha1 else 22] ^= 1
        counts, bad = O.verify(expected)
        left[how]["verify"] = (counts.tolist(), bad.tolist())
        sets[how] = O
    assert set(left["table"]["status"]) <= {0} and left["table"]["counts"][1:3] == [0, 0]
    want_bad = [i for i in (3, 150) if len(objects[i])]
    assert left["table"]["verify"][1] == want_bad
    for key in left["table"]:
        assert left[order][key] == left["table"][key], (call, order, key)
    T, P = sets["table"], sets[order]
    want = reference_order(ext, first) if order == "longest_first" else perm
    assert (P.order_host() == want).all() and (T.order_host() == np.arange(m)).all()
    jf = P.job_first_host()
    assert (T.job_first_host() == first).all() and jf[0] == 0 and jf[-1] == len(ext)
    for r in (0, 1, m // 2, m - 1):
        i = int(want[r])
        a, b = P.jobs_host[int(jf[r]):int(jf[r + 1])], T.jobs_host[int(first[i]):int(first[i + 1])]
        assert a["data"].tolist() == b["data"].tolist() and a["flags"].tolist() == b["flags"].tolist() and a["length"].tolist() == b["length"].tolist()


@pytest.mark.parametrize("stream", ["null", "side"])
def test_stream_order(env, stream):
    """order -> ordered builder -> walk -> efes_objects_results with no host synchronisation in between equals the run
    that synchronises after every step; from a table that lies in device memory, which is never fetched on the way."""
    torch, batch = env["torch"], env["batch"]
    objects = real_objects()
    ext, first = table_of(objects)
    side = torch.cuda.Stream() if stream == "side" else torch.cuda.current_stream()
    got = {}
    with torch.cuda.stream(side):
        ext_d, first_d = _up(torch, ext, np.int64), _up(torch, first, np.int32)
        for how in ("queued", "synchronised"):
            sync = torch.cuda.synchronize if how == "synchronised" else (lambda: None)
            sync()
            O = batch.DeviceObjects.from_table(env["buf"].data_ptr(), ext_d, first_d, ctx=env["ctx"], sha1=True, walk="wide",
                                               order="longest_first")
            sync()
            O.submit()
            sync()
            rec = O._results_call(None, 3, records=True)
            assert not {"first", "last", "jobs_host"} & set(O.__dict__)
            torch.cuda.synchronize()
            got[how] = (rec.cpu().numpy().tobytes(), O._res_counts.cpu().numpy().tolist(), O.sums.cpu().numpy().tobytes(),
                        O.states_host().tobytes(), O.status_host().tolist(), O.order_host().tolist(), O.jobs_host.tobytes() != b"")
    assert got["queued"] == got["synchronised"]
    assert got["queued"][5] == reference_order(ext, first).tolist() and set(got["queued"][4]) == {0}
