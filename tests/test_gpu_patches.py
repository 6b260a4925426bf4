"""GPU parity of efes_patches_table: the device call against its host twin, byte for byte on every output and over
canary-guarded device arrays, at the seams of the sort (tiles of 1024 PATCHes; one, two and three digit passes) and of
the admission (segments of 64, 65 and 129 PATCHes: one lane or the wavefront), on one upload that owns 2^20 PATCHes
and on 2^20 uploads of one PATCH each, with every verdict in one wavefront, on the seeded random logs, and refused
calls that write nothing; then DeviceObjects.from_patches end to end over two rounds, the DEFERRED PATCHes
resubmitted, against hashlib, zlib and the oracle's texts over the admitted bytes.  Bit-exact."""
import ctypes
import hashlib
import zlib

import numpy as np
import pytest

from test_gpu_infos import DeviceGuarded
from test_patches_host import (MASK, OPTIONAL, OUTPUTS, UNKNOWN, automaton, check_against, expected_states, make_log, output_sizes,
                               random_log, random_states, twin, views)

pytestmark = pytest.mark.gpu

POOL_BYTES = 4 << 20
TOP = 1 << 20


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from efes_amd import _lib, batch, hashing
    ctx = hashing.default_context(0)
    buf = torch.empty(POOL_BYTES, dtype=torch.uint8, device="cuda:0")
    ctx.fill_synthetic(buf.data_ptr(), POOL_BYTES, 0x9A7C, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(torch=torch, hashing=hashing, batch=batch, lib=_lib, ctx=ctx, buf=buf, host=buf.cpu().numpy())


def device_table(env, log, offsets, m, states=None, crcs=None, drop=(), expect=0, spoil=None):
    """efes_patches_table over guarded device arrays: what twin() returns.  With expect != 0 the call must be refused
    with that code and leave every output as it was; spoil(req) may change the request first."""
    torch, L = env["torch"], env["lib"]
    n = len(log)
    log_d = DeviceGuarded(torch, 40 * n, np.ascontiguousarray(log))
    offs_d = None if offsets is None else DeviceGuarded(torch, 8 * m, np.ascontiguousarray(offsets, dtype=np.uint64))
    bufs = {k: DeviceGuarded(torch, size) for k, size in output_sizes(m, n).items()}
    st = None if states is None else DeviceGuarded(torch, 104 * m, states)
    cr = None if crcs is None else DeviceGuarded(torch, 4 * m, crcs)
    need = L.lib().efes_patches_table_scratch(m, n)
    scratch = DeviceGuarded(torch, need)
    assert scratch.ptr % 16 == 0 and need >= 16
    req = L.Patches(log=log_d.ptr if n else None, offsets=offs_d.ptr if offs_d is not None and m else None, sha1=st.ptr if st else None,
                    crc32=cr.ptr if cr else None, nobjects=m, npatches=n, **{k: None if k in drop else bufs[k].ptr for k in OUTPUTS})
    args = [scratch.ptr, need]
    if spoil:
        spoil(req, args)
    torch.cuda.synchronize()  # the sentinels and the inputs are in place
    rc = L.lib().efes_patches_table(env["ctx"].handle, ctypes.byref(req), args[0], args[1], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == expect
    assert log_d.fetch().guards_intact() and log_d.body().tobytes() == np.ascontiguousarray(log).tobytes(), "the log is only read"
    assert scratch.fetch().guards_intact(), "the scratch's guards"
    for k, g in list(bufs.items()) + [(k, v) for k, v in (("sha1", st), ("crc32", cr), ("offsets", offs_d)) if v is not None]:
        assert g.fetch().guards_intact(), f"{k}: a guard was written"
        if k in drop or expect:
            if k in OUTPUTS:
                assert (g.body() == 0xA5).all(), f"{k} was written by a call that must not"
    if expect:
        assert (scratch.body() == 0xA5).all(), "a refused call wrote the scratch"
        if st:
            assert (st.body().reshape(m, 104) == states).all() and (cr.body().view(np.uint32) == crcs).all()
        return None
    got = views({k: bufs[k].body().copy() for k in OUTPUTS})
    for k in drop:
        got[k] = None
    got["sha1"] = st.body().reshape(m, 104).copy() if st else None
    got["crc32"] = cr.body().view(np.uint32).copy() if cr else None
    return got


def same_as_twin(env, log, offsets, m, seed=0, drop=()):
    """Both sides from the same inputs: every output and the states, byte for byte."""
    states, crcs = random_states(m, np.random.default_rng(seed))
    want = twin(env["lib"].lib(), log, offsets, m, states, crcs, drop=drop)
    got = device_table(env, log, offsets, m, states, crcs, drop=drop)
    for k in OUTPUTS + ("sha1", "crc32"):
        if want[k] is None:
            assert got[k] is None
            continue
        if got[k].tobytes() != want[k].tobytes():
            bad = np.nonzero(got[k].reshape(-1).view(np.uint8) != want[k].reshape(-1).view(np.uint8))[0]
            raise AssertionError(f"{k}: {bad.size} bytes differ, the first at {int(bad[0])} (m = {m}, n = {len(log)})")
    return got


# ---- the seams of the sort
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_patch_counts_at_the_tile_seams(env, n):
    log, offsets, _ = random_log(7, n, 50 + n)
    got = same_as_twin(env, log, offsets, 7, seed=n)
    check_against(got, automaton(log, offsets, 7))


@pytest.mark.parametrize("m", [1, 2, 255, 256, 257, 65536, 65537])
def test_object_counts_at_the_digit_pass_boundaries(env, m):
    """One digit pass up to 256 objects, two up to 65 536, three beyond; more objects than PATCHes, and the highest
    object index present, so that the top digit counts."""
    n = 200 if m < 65536 else 3000
    log, offsets, _ = random_log(m, n, 7 * m)
    log["object"][n // 2] = m - 1
    log["object"][n // 3] = 0
    same_as_twin(env, log, offsets, m, seed=m)


# ---- the seams of the admission
@pytest.mark.parametrize("longest", [64, 65, 129])
def test_one_long_segment_among_short_ones(env, longest):
    """Object 17 of 40 owns `longest` PATCHes, the others up to three: the switch from one lane to the wavefront."""
    rng = np.random.default_rng(longest)
    owners = np.concatenate((np.full(longest, 17), np.repeat(np.delete(np.arange(40), 17), rng.integers(0, 4, 39))))
    rng.shuffle(owners)
    for seed in (1, 2, 3):  # other mixes of conflicts, restarts and DONEs inside the long segment
        log, offsets, _ = random_log(40, len(owners), 100 * longest + seed, objects=owners)
        same_as_twin(env, log, offsets, 40, seed=seed)
    # exactly `longest` PATCHes: a chain with every seventh PATCH a byte ahead and the DONE on the very last, short objects around it
    records, cur = [(i, 0, 2, UNKNOWN) for i in range(17)], 0
    for k in range(longest):
        if k % 7 == 3:
            records.append((17, cur + 1, 5, UNKNOWN))
        else:
            records.append((17, cur, 5, cur + 5 if k == longest - 1 else UNKNOWN))
            cur += 5
        if k % 9 == 0:
            records.append((18 + k % 22, 0, 1, UNKNOWN))
    got = same_as_twin(env, make_log(records), None, 40)
    assert got["first"][18] - got["first"][17] == longest and int(got["objects"][17]["offset"]) == cur
    assert int(got["objects"][17]["flags"]) == 3 and int(got["objects"][17]["admitted"]) == cur // 5
    # a well-formed chain: one run per step of the wavefront
    records = [(17, 5 * k, 5, UNKNOWN) for k in range(longest)]
    got = same_as_twin(env, make_log(records), None, 40)
    assert got["counts"].tolist() == [longest, 0, 0, 0, 0] and int(got["objects"][17]["offset"]) == 5 * longest


def test_every_verdict_in_one_wavefront(env):
    """The last object's segment of 70 PATCHes, walked by the wavefront, holds all five verdicts, INVALID ones among
    them; and 64 short objects side by side, one per lane, hold them too."""
    tail = [(1, 100, 5, UNKNOWN), (1, 105, 5, UNKNOWN), (1, 7, 5, UNKNOWN), (9, 110, 5, UNKNOWN), (1, 110, 0, UNKNOWN), (0xFFFFFFFF, 0, 0, 0)]
    tail += [(1, 110 + 3 * k, 3, UNKNOWN) for k in range(30)] + [(1, 1, 1, 2), (1, 200, 4, 204), (1, 204, 1, UNKNOWN), (1, 0, 1, UNKNOWN)]
    tail += [(1, 204 + k, 1, UNKNOWN) for k in range(70 - len(tail))]
    got = same_as_twin(env, make_log([(0, 0, 1, 1)] + tail), [0, 100], 2)
    assert len(tail) == 70 and got["counts"].tolist() == [33, 2, 32, 2, 2]
    lanes = []
    for i in range(64):
        lanes += [[(i, 50, 2, UNKNOWN)], [(i, 51, 2, UNKNOWN)], [(i, 50, 2, 52), (i, 52, 1, UNKNOWN)], [(i, 0, 3, UNKNOWN), (i, 0, 3, UNKNOWN)],
                  [(i, 50, 2, UNKNOWN), (70 + i, 0, 0, 0)]][i % 5]
    got = same_as_twin(env, make_log(lanes), np.full(64, 50, np.uint64), 64)
    assert (got["counts"] > 0).all() and got["counts"].tolist() == automaton(make_log(lanes), np.full(64, 50), 64)["counts"].tolist()


def test_one_upload_owns_two_to_the_twenty_patches(env):
    """A table only (no walk, no data): a chain of 2^20 PATCHes, 1 % of them a byte ahead, a DONE 1000 PATCHes before
    the end and the rest behind it."""
    rng = np.random.default_rng(20)
    ahead = rng.random(TOP) < 0.01
    ahead[TOP - 1000] = False
    lengths = np.where(ahead, 7, rng.integers(0, 4097, TOP)).astype(np.uint64)
    taken = np.where(ahead, 0, lengths).astype(np.uint64)
    before = np.uint64(12345) + np.cumsum(taken) - taken
    log = np.zeros(TOP, dtype=env["lib"].PATCH_DTYPE)
    log["length"], log["file_offset"], log["file_length"] = lengths, before + ahead.astype(np.uint64), UNKNOWN
    log["file_length"][TOP - 1000] = before[TOP - 1000] + lengths[TOP - 1000]
    log["data_offset"] = np.arange(TOP, dtype=np.uint64) * np.uint64(4096)
    got = same_as_twin(env, log, [12345], 1)
    nahead = int(ahead[: TOP - 1000].sum())
    assert got["counts"].tolist() == [TOP - 1000 - nahead, nahead, 999, 1, 0] and got["first"].tolist() == [0, TOP]


def test_two_to_the_twenty_uploads_of_one_patch(env):
    """A table only: every upload gets one PATCH, in a shuffled order: three digit passes over 1024 tiles."""
    rng = np.random.default_rng(21)
    stored = rng.integers(1, 1 << 50, TOP).astype(np.uint64)
    order = rng.permutation(TOP)
    kind = rng.random(TOP)
    log = np.zeros(TOP, dtype=env["lib"].PATCH_DTYPE)
    log["object"], log["length"] = order, rng.integers(0, 4097, TOP)
    log["file_offset"] = np.where(kind < 0.05, np.uint64(0), stored[order] + (kind > 0.95).astype(np.uint64))
    log["file_length"] = np.where(kind < 0.5, log["file_offset"] + log["length"], np.uint64(UNKNOWN))
    log["data_offset"] = np.arange(TOP, dtype=np.uint64) * np.uint64(4096)
    got = same_as_twin(env, log, stored, TOP)
    assert (got["first"] == np.arange(TOP + 1)).all() and (got["patch_of"][order] == np.arange(TOP)).all()
    assert (got["counts"][[0, 1, 3]] > 10000).all() and got["counts"][[2, 4]].tolist() == [0, 0]


@pytest.mark.parametrize("m,n", [(257, 4096), (5000, 20000)])
def test_random_logs(env, m, n):
    log, offsets, _ = random_log(m, n, 1000 * m + n)
    got = same_as_twin(env, log, offsets, m, seed=n)
    check_against(got, automaton(log, offsets, m))


def test_optional_outputs_and_empty_logs(env):
    log, offsets, _ = random_log(9, 300, 5)
    for k in range(1 << len(OPTIONAL)):
        same_as_twin(env, log, offsets, 9, drop=tuple(name for b, name in enumerate(OPTIONAL) if k >> b & 1))
    same_as_twin(env, log, None, 9)
    for m in (0, 1, 300, 1025):
        got = same_as_twin(env, make_log([]), None if m == 0 else np.arange(m) + 3, m)
        assert got["first"].tolist() == [0] * (m + 1) and got["counts"].tolist() == [0] * 5


def test_a_refused_call_writes_nothing(env):
    log, offsets, _ = random_log(9, 300, 6)
    states, crcs = random_states(9, np.random.default_rng(6))
    ARG = env["lib"].EFES_ERR_ARG

    def field(name, value):
        return lambda req, args: setattr(req, name, value if value is None or name in ("nobjects", "npatches") else getattr(req, name) + value)

    def scratch(ptr_delta, size):
        def change(req, args):
            args[0] = None if ptr_delta is None else args[0] + ptr_delta
            args[1] = size(args[1])
        return change

    spoils = [field("first", None), field("extents", None), field("log", None), field("answers", 4), field("counts", 2), field("first", 1),
              field("nobjects", TOP + 1), field("npatches", TOP + 1), field("nobjects", 0), field("sha1", 4), field("offsets", 4),
              scratch(None, lambda s: s), scratch(8, lambda s: s), scratch(0, lambda s: s - 1), scratch(0, lambda s: 0)]
    for spoil in spoils:
        device_table(env, log, offsets, 9, states, crcs, expect=ARG, spoil=spoil)


# ---- end to end
def fresh_state_row(lib):
    st = np.zeros(1, lib.SHA1_STATE_DTYPE)
    st["h"] = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
    return st[0]


@pytest.mark.parametrize("walk,with_infos,with_copy", [(None, False, False), ("wide", False, False), ("group4", False, False),
                                                       ("wide", True, False), ("wide", False, True)])
def test_from_patches_end_to_end(env, oracle, walk, with_infos, with_copy):
    """Two rounds over a 4 MiB pool: 65 uploads resumed from the states a prefix left, 600 PATCHes of the random mix;
    round 2 resubmits round 1's DEFERRED PATCHes with the offsets and states round 1 left (offset 0 and fresh states
    behind a DONE).  The running digests at EVERY slot -- DONE slots and refused, zero-length slots included -- the final
    states' `.info` texts and, with copy_to, the gathered bytes against hashlib, zlib and the oracle over the bytes
    the automaton admits."""
    torch, L, DeviceObjects, host = env["torch"], env["lib"], env["batch"].DeviceObjects, env["host"]
    m, n = 65, 600
    mode = L.MODE_GROUP[4] if walk == "group4" else walk
    log, offsets, nbytes = random_log(m, n, 77)
    assert nbytes + 65 * 300 <= POOL_BYTES
    prefix = [(nbytes + 300 * i, (37 * i) % 300) for i in range(m)]  # behind the bodies; object 0 and others start empty
    pre = DeviceObjects(env["buf"].data_ptr(), [[p] for p in prefix], sha1=True, walk="wide", build="device", ctx=env["ctx"])
    pre.run()
    states, crcs = pre.states_host().copy(), pre.crcs.cpu().numpy().view(np.uint32)[:m].copy()
    texts = pre.info_texts(device=True)
    body = [host[o:o + k].tobytes() for o, k in prefix]  # what every upload's digests have seen so far
    cur = offsets.copy()
    for rnd in (1, 2):
        want = automaton(log, cur, m)
        room = torch.full((POOL_BYTES,), 0xEE, dtype=torch.uint8, device="cuda:0") if with_copy else None
        kw = dict(infos=texts) if with_infos and rnd == 1 else dict(states=states, crcs=crcs)
        log_arg, cur_arg = log, cur
        if rnd == 2:  # the log and the offsets as device tensors
            log_arg = torch.from_numpy(np.ascontiguousarray(log).view(np.uint8).reshape(-1)).to("cuda:0")
            cur_arg = torch.from_numpy(cur.view(np.int64)).to("cuda:0")
        objs = DeviceObjects.from_patches(env["buf"].data_ptr(), log_arg, cur_arg, sha1=True, running=True, walk=mode, ctx=env["ctx"],
                                          copy_to=room.data_ptr() if with_copy else None, **kw)
        objs.run()
        assert objs.patch_answers_host().tobytes() == want["answers"].tobytes() and objs.patch_objects_host().tobytes() == want["objects"].tobytes()
        assert objs.patch_counts() == tuple(want["counts"].tolist()) and (objs.patch_of_host() == want["patch_of"]).all()
        assert (objs.status_host() == 0).all(), objs.status_host()
        run_sha, run_crc = objs.running_sha1(), objs.running_crcs().tolist()
        first, ext = want["first"], want["extents"]
        admitted = []
        for i in range(m):
            if want["restarted"][i]:
                body[i] = b""
            mine = b""
            for k in range(int(first[i]), int(first[i + 1])):
                mine += host[int(ext[k]["offset"]):int(ext[k]["offset"]) + int(ext[k]["length"])].tobytes()
                assert run_sha[k] == hashlib.sha1(body[i] + mine).hexdigest(), (rnd, i, k)
                assert run_crc[k] == zlib.crc32(body[i] + mine), (rnd, i, k)
            body[i] += mine
            admitted.append(mine)
        done = np.nonzero(want["answers"]["verdict"] == L.EFES_PATCH_DONE)[0]
        assert len(done) >= 3 or rnd == 2
        for a in done:  # the digests of a DONE PATCH are at its slot
            i, k = int(log["object"][a]), int(want["answers"]["slot"][a])
            assert run_sha[k] == hashlib.sha1(body[i]).hexdigest() and run_crc[k] == zlib.crc32(body[i]), (rnd, i, k)
        if with_copy:
            landed = room.cpu().numpy()
            image = np.full(POOL_BYTES, 0xEE, np.uint8)
            for i, at in enumerate(objs.copy_offsets.tolist()):
                image[at:at + len(admitted[i])] = np.frombuffer(admitted[i], np.uint8)
            assert (landed == image).all(), np.nonzero(landed != image)[0][:8]
        info = objs.info_texts()
        for i in range(0, m, 4):
            d, c = oracle.Sha1(), oracle.Crc32()
            assert d.write(np.frombuffer(body[i], np.uint8)) == 0
            c.write(np.frombuffer(body[i], np.uint8))
            assert info[i][1] == c.marshal_text().encode(), (rnd, i)
            text, nx = d.marshal_text().encode(), len(body[i]) % 64  # x behind nx holds stale bytes that depend on how the Writes were cut
            assert info[i][0][:40 + 2 * nx] == text[:40 + 2 * nx] and info[i][0][168:] == text[168:], (rnd, i)
        # reset() restores the states with the restarts applied: the same run gives the same sums
        objs.reset()
        objs.run()
        assert objs.running_sha1() == run_sha and objs.running_crcs().tolist() == run_crc
        # what the caller keeps for the next log
        states, crcs = objs.states_host().copy(), objs.crcs.cpu().numpy().view(np.uint32)[:m].copy()
        cur = want["objects"]["offset"].copy()
        for i in np.nonzero(want["objects"]["flags"] & L.EFES_PATCH_OBJ_DONE)[0]:
            states[i], crcs[i], cur[i], body[i] = fresh_state_row(L), 0, 0, b""
        again = want["answers"]["verdict"] == L.EFES_PATCH_DEFERRED
        assert again.sum() >= 20 or rnd == 2
        log = log[again]
