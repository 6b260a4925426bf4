"""GPU parity of the chained CRC (efes_crc32_chain): a job with EFES_JOB_CHAIN is the next Write into the
state of the job before it, so one object may lie in many device extents.  States, the 24-byte sums of
every FINALIZE member (the running CRC at that extent's end), status and the untouched sentinels of
invalid members are checked against a serial walk over the job list with zlib (serial_expectation of
tests/test_crc_chain_math.py: zlib of the concatenation, validity job by job), one small case against the
oracle's crc32digest with one write per extent, and unflagged arrays against efes_crc32_batch.  Bit-exact."""
import random
import zlib

import numpy as np
import pytest

from test_crc_chain_math import serial_expectation
from test_gpu_crc_batch import Jobs, _seeded_specs

pytestmark = pytest.mark.gpu

FIN, INIT, SUM_ONLY, CHAIN = 0x1, 0x2, 0x4, 0x8
ARG = -4
BUF_BYTES = 32 << 20


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from efes_amd import _lib, hashing
    from oracle import oracle
    ctx = hashing.default_context(0)
    buf = torch.empty(BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    ctx.fill_synthetic(buf.data_ptr(), BUF_BYTES, 0xC4A17, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(torch=torch, hashing=hashing, lib=_lib, ctx=ctx, oracle=oracle, buf=buf, host=buf.cpu().numpy(),
                T=_lib.EFES_CRC_BATCH_TILE)


def job(off, n, flags, state, **opts):
    """state: index of the CRC state the job names (None: crc32 == NULL); opts: sha1=True."""
    return dict(off=off, n=n, flags=flags, state=state, sha1=opts.get("sha1", False))


class Chains:
    """A device job array over env's buffer with states crc_in[], sentinel sums / status / SHA-1 states."""

    def __init__(self, env, jobs, crc_in):
        torch, lib = env["torch"], env["lib"]
        self.env, self.specs, self.n = env, jobs, len(jobs)
        self.crc_in = [int(c) for c in crc_in]
        n = max(self.n, 1)
        self.crcs = torch.from_numpy(np.array(self.crc_in + [0], dtype=np.uint32).view(np.int32).copy()).to("cuda:0")
        self.sums = torch.full((n * 24,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.status = torch.full((n,), -99, dtype=torch.int32, device="cuda:0")
        self.sha = torch.full((n * 104,), 0x5C, dtype=torch.uint8, device="cuda:0")
        idx = np.arange(self.n, dtype=np.uint64)
        rec = np.zeros(self.n, dtype=lib.JOB_DTYPE)
        rec["data"] = np.uint64(env["buf"].data_ptr()) + np.array([s["off"] for s in jobs], dtype=np.uint64)
        rec["length"] = np.array([s["n"] for s in jobs], dtype=np.uint64)
        rec["flags"] = np.array([s["flags"] for s in jobs], dtype=np.uint32)
        rec["crc32"] = np.array([0 if s["state"] is None else self.crcs.data_ptr() + 4 * s["state"] for s in jobs], dtype=np.uint64)
        rec["sum"] = np.uint64(self.sums.data_ptr()) + idx * np.uint64(24)
        rec["status"] = np.uint64(self.status.data_ptr()) + idx * np.uint64(4)
        rec["sha1"] = np.array([self.sha.data_ptr() + 104 * j if s["sha1"] else 0 for j, s in enumerate(jobs)], dtype=np.uint64)
        self.jobs = torch.from_numpy(rec.view(np.uint8).copy()).to("cuda:0") if self.n else torch.zeros(56, dtype=torch.uint8, device="cuda:0")
        self.scratch_bytes = env["hashing"].crc32_chain_scratch(self.n)
        self.scratch = torch.empty(max(self.scratch_bytes, 16), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def run(self, stream="current"):
        s = self.env["torch"].cuda.current_stream().cuda_stream if stream == "current" else stream
        self.env["ctx"].crc32_chain(self.jobs.data_ptr(), self.n, self.scratch.data_ptr(), self.scratch_bytes, s)

    def results(self):
        self.env["torch"].cuda.synchronize()
        return (self.crcs.cpu().numpy().view(np.uint32)[:len(self.crc_in)].copy(),
                self.sums.cpu().numpy()[:24 * self.n].reshape(self.n, 24).copy(), self.status.cpu().numpy()[:self.n].copy(),
                self.sha.cpu().numpy().copy())

    def expected(self):
        """(states, sums, status) by zlib; an invalid member keeps its sentinels."""
        host = self.env["host"]
        model = [dict(data=host[s["off"]:s["off"] + s["n"]], flags=s["flags"], state=s["state"], sha1=s["sha1"]) for s in self.specs]
        states, sums, status = serial_expectation(model, dict(enumerate(self.crc_in)))
        esums = np.full((self.n, 24), 0xA5, dtype=np.uint8)
        for j, c in enumerate(sums):
            if c is not None:
                esums[j] = np.frombuffer(bytes(20) + c.to_bytes(4, "big"), dtype=np.uint8)
        return (np.array([states[k] for k in range(len(self.crc_in))], dtype=np.uint32), esums, np.array(status, dtype=np.int32))

    def check(self, what=""):
        crcs, sums, status, sha = self.results()
        ecrcs, esums, estatus = self.expected()
        bad = np.nonzero(status != estatus)[0]
        assert bad.size == 0, (what, "status", [(int(j), self.specs[j], int(status[j]), int(estatus[j])) for j in bad[:5]])
        bad = np.nonzero((sums != esums).any(axis=1))[0]
        assert bad.size == 0, (what, "sum", [(int(j), self.specs[j], bytes(sums[j]).hex(), bytes(esums[j]).hex()) for j in bad[:5]])
        bad = np.nonzero(crcs != ecrcs)[0]
        assert bad.size == 0, (what, "state", [(int(k), hex(crcs[k]), hex(ecrcs[k])) for k in bad[:5]])
        assert (sha == 0x5C).all(), (what, "a SHA-1 state was written")
        return estatus


def test_unflagged_array_equals_the_batch_call(env):
    """The 300 seeded jobs of test_same_bytes_as_hash_submit through both calls on copies of the
    in-states: states, 24-byte sums, status and the SHA-1 sentinel byte-identical."""
    torch = env["torch"]
    specs = _seeded_specs(random.Random(300), 300, 2 << 20)
    A, B = Jobs(env, specs), Jobs(env, specs)
    nbytes = env["hashing"].crc32_chain_scratch(B.n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda:0")
    A.batch()
    env["ctx"].crc32_chain(B.jobs.data_ptr(), B.n, scratch.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    for a, b, what in zip(A.results(), B.results(), ("crc", "sum", "status", "sha1")):
        assert (a == b).all(), (what, np.nonzero(a != b))
    B.check()


def _array_with_chains(rng, count, chains, lengths):
    """count jobs, chains of one except the inclusive index ranges in `chains`; state k belongs to chain k."""
    start = {a: b for a, b in chains}
    jobs, crc_in, j = [], [], 0
    while j < count:
        end = start.get(j, j)
        for i in range(j, end + 1):
            n = rng.choice(lengths)
            flags = (CHAIN if i > j else rng.choice([0, INIT])) | rng.choice([0, FIN])
            jobs.append(job(rng.randrange(0, BUF_BYTES - n), n, flags, len(crc_in)))
        crc_in.append(rng.getrandbits(32))
        j = end + 1
    return jobs, crc_in


@pytest.mark.parametrize("count,chains", [
    (2200, [(40, 63), (64, 100), (1000, 1023), (1024, 1060), (2000, 2047), (2048, 2100)]),
    (1300, [(1000, 1100)]),
], ids=["ends-and-starts-at-64-1024-2048", "across-1024"])
def test_chains_at_the_scan_boundaries(env, count, chains):
    """Chains that end and start exactly at the wave (63/64) and block (1023/1024, 2047/2048) boundaries
    of the scan, and one that covers jobs 1000-1100; chains of one between them."""
    jobs, crc_in = _array_with_chains(random.Random(count), count, chains, [0, 5, 40, 300, 5000, 70000])
    C = Chains(env, jobs, crc_in)
    C.run()
    assert (C.check() == 0).all()


def test_chain_over_69_blocks(env):
    """One chain of 70 000 members of 0-40 bytes with runs of consecutive empty members, chains of one
    before and behind it: the carry crosses every block."""
    rng = random.Random(69)
    lengths = []
    while len(lengths) < 70000:
        if rng.random() < 0.01:
            lengths += [0] * rng.choice([3, 70, 130])
        lengths.append(rng.randrange(0, 41))
    lengths = lengths[:70000]
    jobs = [job(rng.randrange(0, 1 << 22), rng.randrange(0, 41), rng.choice([0, INIT, FIN]), k) for k in range(5)]
    jobs += [job(rng.randrange(0, 1 << 22), n, (CHAIN if i else 0) | (FIN if rng.random() < 0.3 else 0), 5) for i, n in enumerate(lengths)]
    jobs += [job(rng.randrange(0, 1 << 22), rng.randrange(0, 41), rng.choice([0, INIT, FIN]), 6 + k) for k in range(5)]
    assert (len(jobs) + 1023) // 1024 == 69
    C = Chains(env, jobs, [rng.getrandbits(32) for _ in range(11)])
    C.run()
    assert (C.check() == 0).all()


def test_byte_boundaries_inside_a_chain(env):
    """Members of every length around the 16-byte piece and the tile at four misalignments inside one
    chain, once from a fresh head and once from a mid-stream head; FINALIZE on every member."""
    T = env["T"]
    members, at = [], 0
    for n in [0, 1, 15, 16, 17, 4097, T - 1, T, T + 1, 3 * T + 17]:
        for off in (0, 1, 7, 15):
            members.append((at + off, n))
            at += (n + 16 + 4095) // 4096 * 4096
    assert at <= BUF_BYTES and len(members) == 40
    random.Random(40).shuffle(members)
    jobs = []
    for state, head_flags in ((0, INIT), (1, 0)):
        jobs += [job(off, n, FIN | (CHAIN if i else head_flags), state) for i, (off, n) in enumerate(members)]
    C = Chains(env, jobs, [0x0BADF00D, 0x13572468])
    C.run()
    assert (C.check() == 0).all()
    crcs = C.results()[0]
    whole = b"".join(env["host"][off:off + n].tobytes() for off, n in members)
    assert [int(c) for c in crcs] == [zlib.crc32(whole), zlib.crc32(whole, 0x13572468)]


def test_running_sums(env):
    """FINALIZE on every member of 64 chains of 1-40 members: every sum is the prefix CRC big-endian
    behind 20 zero bytes, and only the object's final value lands in the state.  The first chain also
    against the oracle's crc32digest, one write per extent."""
    rng = random.Random(64)
    host, oracle = env["host"], env["oracle"]
    jobs, crc_in, extents = [], [], []
    for k in range(64):
        ext = []
        for i in range(rng.randrange(1, 41)):
            n = rng.choice([0, 1, 33, 1000, 70000, rng.randrange(0, 200000)])
            ext.append((rng.randrange(0, BUF_BYTES - n), n))
            jobs.append(job(ext[-1][0], n, FIN | (CHAIN if i else (INIT if k % 2 else 0)), k))
        extents.append(ext)
        crc_in.append(rng.getrandbits(32))
    C = Chains(env, jobs, crc_in)
    C.run()
    assert (C.check() == 0).all()
    crcs, sums, _, _ = C.results()
    j = 0
    for k, ext in enumerate(extents):
        run = 0 if k % 2 else crc_in[k]
        for off, n in ext:
            run = zlib.crc32(host[off:off + n], run)
            assert bytes(sums[j]) == bytes(20) + run.to_bytes(4, "big"), (k, j)
            j += 1
        assert int(crcs[k]) == run
    o = oracle.Crc32()
    o.st.crc = crc_in[0]
    for j, (off, n) in enumerate(extents[0]):
        o.write(host[off:off + n].tobytes())
        assert int.from_bytes(bytes(sums[j][20:]), "big") == o.sum32(), j
    assert int(crcs[0]) == o.sum32()


def _invalid_cases():
    """name -> (the jobs of the case over states 1 (and 2, the "other" state), their statuses)."""
    def m(flags, state=1, **o):
        return dict(flags=flags, state=state, **o)
    OK = 0
    return {
        "chain-on-job-0": ([m(CHAIN | FIN), m(CHAIN | FIN), m(FIN), m(CHAIN | FIN)], [ARG, ARG, OK, OK]),
        "another-state": ([m(INIT | FIN), m(CHAIN | FIN), m(CHAIN | FIN, 2), m(CHAIN | FIN, 2), m(CHAIN | FIN)], [OK, OK, ARG, ARG, ARG]),
        "null-state": ([m(FIN), m(CHAIN | FIN, None), m(CHAIN | FIN)], [OK, ARG, ARG]),
        "chain-with-sha1": ([m(INIT), m(CHAIN | FIN), m(CHAIN | FIN, sha1=True), m(CHAIN | FIN)], [OK, OK, ARG, ARG]),
        "chain-init": ([m(FIN), m(CHAIN | INIT | FIN), m(CHAIN | FIN)], [OK, ARG, ARG]),
        "chain-sum-only": ([m(FIN), m(CHAIN | FIN), m(CHAIN | SUM_ONLY | FIN), m(CHAIN | FIN)], [OK, OK, ARG, ARG]),
        "behind-sum-only-head": ([m(SUM_ONLY | FIN), m(CHAIN | FIN), m(CHAIN | FIN)], [OK, ARG, ARG]),
        "sha1-head": ([m(INIT | FIN, sha1=True), m(CHAIN | FIN), m(CHAIN | FIN)], [ARG, ARG, ARG]),
        "middle-of-ten": ([m(CHAIN | FIN if i else FIN, sha1=(i == 5)) for i in range(10)], [OK] * 5 + [ARG] * 5),
    }


@pytest.mark.parametrize("case", list(_invalid_cases()))
def test_invalid_members(env, case):
    """An invalid member and what follows it in its chain get EFES_ERR_ARG and keep their sentinels; the
    state holds the CRC of the valid prefix; the chains before and behind are right."""
    host = env["host"]
    members, statuses = _invalid_cases()[case]
    rng = random.Random(case)

    def place(parts):
        out = []
        for p in parts:
            n = 0 if p["flags"] & SUM_ONLY else rng.choice([0, 7, 500, 70001])  # SUM_ONLY jobs are zero-length
            out.append(job(rng.randrange(0, BUF_BYTES - n), n, p["flags"], p["state"], sha1=p.get("sha1", False)))
        return out
    before = place([dict(flags=INIT | FIN, state=0), dict(flags=CHAIN, state=0), dict(flags=CHAIN | FIN, state=0)])
    after = place([dict(flags=FIN, state=3), dict(flags=CHAIN | FIN, state=3), dict(flags=CHAIN, state=3)])
    mid = place(members)
    if case == "chain-on-job-0":
        before = []
    crc_in = [rng.getrandbits(32) for _ in range(4)]
    C = Chains(env, before + mid + after, crc_in)
    C.run()
    estatus = C.check(case)
    assert estatus.tolist() == [0] * len(before) + statuses + [0] * 3
    crcs, sums, status, _ = C.results()
    assert status.tolist() == estatus.tolist()
    for j, s in enumerate(statuses):  # sentinels of the invalid members
        assert s == 0 or (sums[len(before) + j] == 0xA5).all()
    # state 1: the valid prefix of the case's chain(s), Write after Write; state 2 is never written
    run, wrote = crc_in[1], False
    for s, spec in zip(statuses, mid):
        if s == 0 and spec["state"] == 1 and not spec["flags"] & SUM_ONLY:
            run = zlib.crc32(host[spec["off"]:spec["off"] + spec["n"]], 0 if spec["flags"] & INIT else run)
            wrote = True
    assert int(crcs[1]) == run and int(crcs[2]) == crc_in[2], (case, wrote)


def test_composition(env):
    """An object split between two calls on one stream (the second call's head is unflagged and
    mid-stream), and efes_crc32_span followed by a chain on the same state: zlib of the whole."""
    torch, T, host = env["torch"], env["T"], env["host"]
    rng = random.Random(17)
    objects = []
    for _ in range(32):
        ext = []
        for _ in range(rng.randrange(2, 12)):
            n = rng.choice([0, 1, 17, 4096, T, 2 * T + 5, rng.randrange(0, 3 * T)])
            ext.append((rng.randrange(0, BUF_BYTES - n), n))
        objects.append((ext, rng.randrange(1, len(ext))))
    first = Chains(env, [job(off, n, CHAIN if i else INIT, k) for k, (ext, cut) in enumerate(objects) for i, (off, n) in enumerate(ext[:cut])],
                   [rng.getrandbits(32) for _ in objects])
    second = Chains(env, [job(off, n, (CHAIN if i else 0) | FIN, k) for k, (ext, cut) in enumerate(objects) for i, (off, n) in enumerate(ext[cut:])],
                    [0] * len(objects))
    rec = second.jobs.cpu().numpy().view(env["lib"].JOB_DTYPE).copy()
    rec["crc32"] = rec["crc32"] - np.uint64(second.crcs.data_ptr()) + np.uint64(first.crcs.data_ptr())  # the first call's states
    second.jobs.copy_(torch.from_numpy(rec.view(np.uint8)))
    torch.cuda.synchronize()
    first.run()
    second.run()
    crcs = first.results()[0]
    want = [zlib.crc32(b"".join(host[off:off + n].tobytes() for off, n in ext)) for ext, _ in objects]
    assert [int(c) for c in crcs] == want
    assert (second.results()[2] == 0).all()
    # span, then a chain, on one state
    a, parts = (1 << 20) + 7, [3 * T + 11, 0, 5, T]
    offs = [9 + a + sum(parts[:i]) for i in range(len(parts))]
    C = Chains(env, [job(off, n, CHAIN if i else 0, 0) for i, (off, n) in enumerate(zip(offs, parts))], [0x2468ACE0])
    env["ctx"].crc32_span(env["buf"].data_ptr() + 9, a, C.crcs.data_ptr(), torch.cuda.current_stream().cuda_stream)
    C.run()
    assert int(C.results()[0][0]) == zlib.crc32(host[9:9 + a + sum(parts)], 0x2468ACE0)


def _seeded_chains(rng, nchains):
    jobs, crc_in = [], []
    for k in range(nchains):
        for i in range(rng.randrange(1, 9)):
            n = int(2 ** rng.uniform(0, 20)) - 1
            jobs.append(job(rng.randrange(0, BUF_BYTES - n), n, (CHAIN if i else rng.choice([0, INIT])) | rng.choice([0, FIN]), k))
        crc_in.append(rng.getrandbits(32))
    return jobs, crc_in


def test_streams(env):
    """Two torch streams with a scratch each, and the NULL (context) stream, interleaved."""
    torch = env["torch"]
    rng = random.Random(19)
    sets = [Chains(env, *_seeded_chains(rng, 12)) for _ in range(3)]
    streams = [torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0"), None]
    init = [C.crcs.clone() for C in sets]
    torch.cuda.synchronize()
    for rep in range(3):
        for C, s, c in zip(sets, streams, init):
            if s is None:
                C.crcs.copy_(c)
                torch.cuda.synchronize()  # the context's own stream is not ordered with torch's
                C.run(None)
            else:
                with torch.cuda.stream(s):
                    C.crcs.copy_(c)
                    C.run(s.cuda_stream)
        env["ctx"].sync()
        for C in sets:
            C.check(rep)


def test_arguments(env):
    """The batch call's cases against the chain scratch size: njobs == 0 is OK and touches nothing; too
    many jobs and a NULL, short or misaligned scratch are EFES_ERR_ARG and launch nothing (a scratch of
    the batch call's size is short): the sentinel state is unchanged after a sync."""
    torch, lib = env["torch"], env["lib"]
    L, ctx = lib.lib(), env["ctx"]
    C = Chains(env, [job(0, 1000, FIN, 0), job(1000, 24, CHAIN | FIN, 0)], [0xDEADBEEF])
    s = torch.cuda.current_stream().cuda_stream
    jp, sp, sb = C.jobs.data_ptr(), C.scratch.data_ptr(), C.scratch_bytes
    big = torch.empty(sb + 64, dtype=torch.uint8, device="cuda:0")
    assert L.efes_crc32_chain(ctx.handle, jp, 0, sp, sb, s) == lib.EFES_OK
    assert L.efes_crc32_chain(ctx.handle, None, 0, None, 0, s) == lib.EFES_OK
    assert env["hashing"].crc32_batch_scratch(2) < sb
    for args in [(jp, lib.EFES_CRC_BATCH_MAX_JOBS + 1, sp, sb), (jp, 2, None, sb), (jp, 2, sp, sb - 1),
                 (jp, 2, sp, env["hashing"].crc32_batch_scratch(2)), (jp, 2, big.data_ptr() + 8, sb + 56), (None, 2, sp, sb)]:
        assert L.efes_crc32_chain(ctx.handle, *args, s) == lib.EFES_ERR_ARG, args
    torch.cuda.synchronize()
    crcs, sums, status, _ = C.results()
    assert int(crcs[0]) == 0xDEADBEEF and (sums == 0xA5).all() and (status == -99).all()
    C.run()
    C.check()


def test_device_objects(env):
    """DeviceObjects: per-object and running CRCs against zlib, fresh and from given states; reset and
    rerun keep the scratch."""
    from efes_amd.batch import DeviceObjects
    T, host = env["T"], env["host"]
    rng = random.Random(23)
    objects = [[(rng.randrange(0, 1 << 24), rng.choice([0, 1, 4097, T, 3 * T + 5, rng.randrange(0, 1 << 20)])) for _ in range(k)]
               for k in (1, 9, 0, 33, 2)]
    crcs = np.array([rng.getrandbits(32) for _ in objects], dtype=np.uint32)
    for fresh in (True, False):
        want_run = []
        for ext, c in zip(objects, crcs):
            run = 0 if fresh else int(c)
            for off, n in ext:
                run = zlib.crc32(host[off:off + n], run)
                want_run.append(run)
        want = [zlib.crc32(b"".join(host[off:off + n].tobytes() for off, n in ext), 0 if fresh else int(c)) if ext else int(c)
                for ext, c in zip(objects, crcs)]
        d = DeviceObjects(env["buf"].data_ptr(), objects, crcs=crcs, fresh=fresh, running=True, ctx=env["ctx"])
        d.run()
        assert (d.status_host() == 0).all() and d.status_host().size == sum(len(o) for o in objects)
        assert d.crc_sum().tolist() == want and d.running_crcs().tolist() == want_run
        scratch = d._scratch.data_ptr()
        d.reset()
        d.run()  # the scratch is kept
        assert d._scratch.data_ptr() == scratch and d.crc_sum().tolist() == want
        last = DeviceObjects(env["buf"].data_ptr(), objects, crcs=crcs, fresh=fresh, ctx=env["ctx"])
        last.run()
        assert last.crc_sum().tolist() == want
        with pytest.raises(ValueError):
            last.running_crcs()
