"""GPU parity of the batched CRC (efes_crc32_batch, ABI 8): the CRC-only jobs of a device job array,
their bytes dealt to the whole GPU in tiles of T = EFES_CRC_BATCH_TILE, must leave exactly what
efes_hash_submit leaves for the same jobs -- states, 24-byte sums, status -- and equal crc32.go's serial
Write (the oracle's C restatement, zlib.crc32 where the oracle would take long).  Bit-exact."""
import random
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIN, INIT, SUM_ONLY = 0x1, 0x2, 0x4
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
    ctx.fill_synthetic(buf.data_ptr(), BUF_BYTES, 0xBA7C4, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(torch=torch, hashing=hashing, lib=_lib, ctx=ctx, oracle=oracle, buf=buf, host=buf.cpu().numpy(),
                T=_lib.EFES_CRC_BATCH_TILE)


class Jobs:
    """A device job array over env's buffer.  spec: (off, n, crc_in, flags) plus the optional keys
    crc (False: crc32 == NULL), status (False: status == NULL), sha1 (True: a SHA-1 state too)."""

    def __init__(self, env, specs, data_ptr=None):
        torch, lib = env["torch"], env["lib"]
        self.env, self.n = env, len(specs)
        self.specs = [{**dict(off=s[0], n=s[1], crc_in=s[2], flags=s[3], crc=True, status=True, sha1=False),
                       **(s[4] if len(s) > 4 else {})} for s in specs]
        n = max(self.n, 1)
        crc_in = np.array([s["crc_in"] for s in self.specs] + [0] * (n - self.n), dtype=np.uint32)
        self.crcs = torch.from_numpy(crc_in.view(np.int32).copy()).to("cuda:0")
        self.sums = torch.full((n * 24,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.status = torch.full((n,), -99, dtype=torch.int32, device="cuda:0")
        self.sha = torch.full((n * 104,), 0x5C, dtype=torch.uint8, device="cuda:0")
        jobs = np.zeros(self.n, dtype=lib.JOB_DTYPE)
        base = env["buf"].data_ptr() if data_ptr is None else data_ptr
        for j, s in enumerate(self.specs):
            jobs[j]["data"] = base + s["off"]
            jobs[j]["length"] = s["n"]
            jobs[j]["flags"] = s["flags"]
            jobs[j]["crc32"] = self.crcs.data_ptr() + 4 * j if s["crc"] else 0
            jobs[j]["sum"] = self.sums.data_ptr() + 24 * j
            jobs[j]["status"] = self.status.data_ptr() + 4 * j if s["status"] else 0
            jobs[j]["sha1"] = self.sha.data_ptr() + 104 * j if s["sha1"] else 0
        self.jobs = torch.from_numpy(jobs.view(np.uint8).copy()).to("cuda:0") if self.n else torch.zeros(56, dtype=torch.uint8, device="cuda:0")
        nbytes = env["hashing"].crc32_batch_scratch(self.n)
        self.scratch = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda:0")
        self.scratch_bytes = nbytes
        torch.cuda.synchronize()

    def batch(self, stream="current"):
        torch = self.env["torch"]
        s = torch.cuda.current_stream().cuda_stream if stream == "current" else stream
        self.env["ctx"].crc32_batch(self.jobs.data_ptr(), self.n, self.scratch.data_ptr(), self.scratch_bytes, s)

    def submit(self):
        torch = self.env["torch"]
        self.env["ctx"].submit(self.jobs.data_ptr(), self.n, torch.cuda.current_stream().cuda_stream, self.env["lib"].MODE_AUTO)

    def results(self):
        self.env["torch"].cuda.synchronize()
        return (self.crcs.cpu().numpy().view(np.uint32)[:self.n].copy(), self.sums.cpu().numpy()[:24 * self.n].reshape(self.n, 24).copy(),
                self.status.cpu().numpy()[:self.n].copy(), self.sha.cpu().numpy().copy())

    def expected(self):
        """(crcs, sums, status) by zlib, per the contract of efes_hash.h."""
        host = self.env["host"]
        crcs, sums, status = [], [], []
        for s in self.specs:
            if s["sha1"]:
                crcs.append(s["crc_in"]); sums.append(bytes([0xA5]) * 24); status.append(-4 if s["status"] else -99)
                continue
            out = zlib.crc32(host[s["off"]:s["off"] + s["n"]], 0 if s["flags"] & INIT else s["crc_in"])
            crcs.append(s["crc_in"] if (s["flags"] & SUM_ONLY or not s["crc"]) else out)
            sums.append(bytes(20) + (out if s["crc"] else 0).to_bytes(4, "big") if s["flags"] & FIN else bytes([0xA5]) * 24)
            status.append(0 if s["status"] else -99)
        return np.array(crcs, dtype=np.uint32), np.frombuffer(b"".join(sums), dtype=np.uint8).reshape(-1, 24), np.array(status, dtype=np.int32)

    def check(self, what=""):
        crcs, sums, status, sha = self.results()
        ecrcs, esums, estatus = self.expected()
        bad = np.nonzero(crcs != ecrcs)[0]
        assert bad.size == 0, (what, "crc", [(int(j), self.specs[j], hex(crcs[j]), hex(ecrcs[j])) for j in bad[:5]])
        bad = np.nonzero((sums != esums).any(axis=1))[0]
        assert bad.size == 0, (what, "sum", [(int(j), self.specs[j], bytes(sums[j]).hex(), bytes(esums[j]).hex()) for j in bad[:5]])
        assert (status == estatus).all(), (what, "status", np.nonzero(status != estatus)[0][:5])
        assert (sha == 0x5C).all(), (what, "a SHA-1 state was written")


def test_boundaries_one_launch(env):
    """Every length around the 16-byte piece, the tile and several tiles, at four misalignments, from
    fresh and mid-stream states, in ONE launch; against the oracle's crc32digest."""
    T, oracle, host = env["T"], env["oracle"], env["host"]
    lengths = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, T - 1, T, T + 1, T + 64 * 7 + 5,
               2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 17, 8 * T + 13]
    rng = random.Random(21)
    specs, at = [], 0
    for n in lengths:
        for off in (0, 1, 7, 15):
            specs.append((at + off, n, rng.choice([0, 0xFFFFFFFF, rng.getrandbits(32)]), 0))
            at += (n + 16 + 4095) // 4096 * 4096
    assert at <= BUF_BYTES and len(specs) == 92
    J = Jobs(env, specs)
    J.batch()
    crcs = J.results()[0]
    for j, (off, n, crc_in, _) in enumerate(specs):
        o = oracle.Crc32()
        o.st.crc = crc_in
        o.write(host[off:off + n].tobytes())
        assert int(crcs[j]) == o.sum32(), (n, off % 4096, hex(crc_in), hex(int(crcs[j])), hex(o.sum32()))
    J.check()


def _seeded_specs(rng, count, max_bytes):
    specs = []
    for _ in range(count):
        n = int(2 ** rng.uniform(0, np.log2(max_bytes))) - 1
        off = rng.randrange(0, BUF_BYTES - n)
        opts = {}
        if rng.random() < 0.1:
            opts["crc"] = False
        if rng.random() < 0.15:
            opts["status"] = False
        specs.append((off, n, rng.getrandbits(32), rng.choice([0, INIT, FIN, INIT | FIN]), opts))
    return specs


def test_same_bytes_as_hash_submit(env):
    """300 seeded jobs, lengths log-uniform up to 2 MiB, flags mixed, some without a CRC state or a
    status: states, the whole 24-byte sums and status byte-identical to efes_hash_submit(MODE_AUTO)
    on a copy of the same in-states; the CRCs against zlib too."""
    specs = _seeded_specs(random.Random(300), 300, 2 << 20)
    A, B = Jobs(env, specs), Jobs(env, specs)
    A.batch()
    B.submit()
    ra, rb = A.results(), B.results()
    for a, b, what in zip(ra, rb, ("crc", "sum", "status", "sha1")):
        assert (a == b).all(), (what, np.nonzero(a != b))
    A.check()


def test_sum_semantics(env):
    """Zero-length FINALIZE jobs and SUM_ONLY jobs on mid-stream states: the sums are the states'
    CRCs big-endian behind 20 zero bytes, and SUM_ONLY leaves the state bytes untouched."""
    rng = random.Random(3)
    specs = []
    for k in range(40):
        crc_in = rng.getrandbits(32)
        specs.append((16 * k + k % 5, 0, crc_in, FIN | (SUM_ONLY if k % 2 else 0)))
    specs.append((0, 0, 0x01020304, FIN | INIT))  # NewCRC32IEEE(): sum of nothing
    specs.append((64, 0, 0x0A0B0C0D, FIN | SUM_ONLY, dict(crc=False)))  # nothing to sum: zeros
    J = Jobs(env, specs)
    J.batch()
    crcs, sums, _, _ = J.results()
    for j, s in enumerate(specs[:40]):
        assert bytes(sums[j]) == bytes(20) + s[2].to_bytes(4, "big") and int(crcs[j]) == s[2]
    assert bytes(sums[40]) == bytes(24) and int(crcs[40]) == 0
    assert bytes(sums[41]) == bytes(24) and int(crcs[41]) == 0x0A0B0C0D
    J.check()


def test_sha1_job_in_the_batch(env):
    """Jobs with sha1 != NULL among valid ones: status EFES_ERR_ARG, their states and sum buffers keep
    the sentinel pattern, every other job is right."""
    T = env["T"]
    rng = random.Random(4)
    specs = []
    for k in range(24):
        n = rng.choice([0, 40, 5000, T + 3, 3 * T + 100])
        opts = dict(sha1=True) if k in (0, 7, 8, 23) else {}
        specs.append((rng.randrange(0, 1 << 20), n, rng.getrandbits(32), rng.choice([0, FIN]), opts))
    J = Jobs(env, specs)
    J.batch()
    _, _, status, _ = J.results()
    assert [int(s) for s in status[[0, 7, 8, 23]]] == [env["lib"].EFES_ERR_ARG] * 4
    J.check()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_skew_one_big_job_among_small(env, where):
    """One 24 MiB job among 2 000 of 0-300 bytes with runs of consecutive empty jobs (the walk from a
    job to the next one with tiles crosses more than one wave's worth of them); against zlib."""
    rng = random.Random(5)
    small = []
    while len(small) < 2000:
        if rng.random() < 0.02:
            small += [(rng.randrange(0, 1 << 20), rng.choice([0, 3, 15]), rng.getrandbits(32), 0) for _ in range(rng.choice([70, 130, 200]))]
        small.append((rng.randrange(0, 1 << 20), rng.randrange(0, 301), rng.getrandbits(32), rng.choice([0, FIN])))
    small = small[:2000]
    big = (5, (24 << 20) + 77, 0x1357, FIN)
    at = {"first": 0, "middle": 1000, "last": 2000}[where]
    J = Jobs(env, small[:at] + [big] + small[at:])
    J.batch()
    J.check(where)


def test_skew_many_tiny_jobs(env):
    """65 537 jobs of 0-40 bytes: more than 64 blocks of the prefix sum, most jobs without a tile."""
    rng = random.Random(6)
    specs = [(rng.randrange(0, 1 << 22), rng.randrange(0, 41), rng.getrandbits(32), 0) for _ in range(65537)]
    J = Jobs(env, specs)
    J.batch()
    J.check()


def test_composition(env):
    """Each job split at a random point into two calls on one stream == one call; and efes_crc32_span
    followed by efes_crc32_batch on the same state == zlib of the concatenation."""
    torch, T, host = env["torch"], env["T"], env["host"]
    rng = random.Random(7)
    whole = [(rng.randrange(0, 1 << 20), rng.choice([1, 17, 4096, T, 2 * T + 5, rng.randrange(0, 5 * T)]), rng.getrandbits(32), 0)
             for _ in range(64)]
    cuts = [rng.randrange(0, s[1] + 1) for s in whole]
    one = Jobs(env, whole)
    one.batch()
    first = Jobs(env, [(s[0], c, s[2], 0) for s, c in zip(whole, cuts)])
    first.batch()
    second = Jobs(env, [(s[0] + c, s[1] - c, 0, 0) for s, c in zip(whole, cuts)])
    second.jobs.copy_(torch.from_numpy(_retarget(env, second, first)))  # the second halves write the first halves' states
    torch.cuda.synchronize()
    second.batch()
    torch.cuda.synchronize()
    assert (first.crcs.cpu().numpy().view(np.uint32)[:64] == one.results()[0]).all()
    one.check()
    # span, then batch, on one state
    a, b = (1 << 20) + 7, 3 * T + 11
    st = torch.tensor([0x2468ACE0], dtype=torch.int64, device="cuda:0")
    s = torch.cuda.current_stream().cuda_stream
    J = Jobs(env, [(9 + a, b, 0, 0)])
    jobs = J.jobs.cpu().numpy().view(env["lib"].JOB_DTYPE).copy()
    jobs[0]["crc32"] = st.data_ptr()
    J.jobs.copy_(torch.from_numpy(jobs.view(np.uint8)))
    torch.cuda.synchronize()
    env["ctx"].crc32_span(env["buf"].data_ptr() + 9, a, st.data_ptr(), s)
    J.batch()
    torch.cuda.synchronize()
    assert int(st.item()) & 0xFFFFFFFF == zlib.crc32(host[9:9 + a + b], 0x2468ACE0)


def _retarget(env, jobs, onto):
    """jobs' records with the crc32 pointers of `onto` (same job count)."""
    rec = jobs.jobs.cpu().numpy().view(env["lib"].JOB_DTYPE).copy()
    rec["crc32"] = onto.crcs.data_ptr() + 4 * np.arange(jobs.n, dtype=np.uint64)
    return rec.view(np.uint8)


def test_streams(env):
    """Two torch streams with a scratch each, and the NULL (context) stream, interleaved."""
    torch = env["torch"]
    rng = random.Random(9)
    sets = [Jobs(env, _seeded_specs(rng, 40, 1 << 20)) for _ in range(3)]
    streams = [torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0"), None]
    init = [J.crcs.clone() for J in sets]
    torch.cuda.synchronize()
    for rep in range(3):
        for J, s, c in zip(sets, streams, init):
            if s is None:
                J.crcs.copy_(c)
                torch.cuda.synchronize()  # the context's own stream is not ordered with torch's
                J.batch(None)
            else:
                with torch.cuda.stream(s):
                    J.crcs.copy_(c)
                    J.batch(s.cuda_stream)
        env["ctx"].sync()
        for J in sets:
            J.check(rep)


def test_arguments(env):
    """njobs == 0 is OK and touches nothing; too many jobs and a NULL, short or misaligned scratch are
    EFES_ERR_ARG and launch nothing: the sentinel state is unchanged after a sync."""
    torch, lib = env["torch"], env["lib"]
    L, ctx = lib.lib(), env["ctx"]
    J = Jobs(env, [(0, 1000, 0xDEADBEEF, FIN)])
    s = torch.cuda.current_stream().cuda_stream
    jp, sp, sb = J.jobs.data_ptr(), J.scratch.data_ptr(), J.scratch_bytes
    big = torch.empty(sb + 64, dtype=torch.uint8, device="cuda:0")
    assert L.efes_crc32_batch(ctx.handle, jp, 0, sp, sb, s) == lib.EFES_OK
    assert L.efes_crc32_batch(ctx.handle, None, 0, None, 0, s) == lib.EFES_OK
    for args in [(jp, lib.EFES_CRC_BATCH_MAX_JOBS + 1, sp, sb), (jp, 1, None, sb), (jp, 1, sp, sb - 1),
                 (jp, 1, big.data_ptr() + 8, sb + 56), (None, 1, sp, sb)]:
        assert L.efes_crc32_batch(ctx.handle, *args, s) == lib.EFES_ERR_ARG, args
    torch.cuda.synchronize()
    crcs, sums, status, _ = J.results()
    assert int(crcs[0]) == 0xDEADBEEF and (sums == 0xA5).all() and int(status[0]) == -99
    J.batch()
    J.check()


def test_device_batch_run_crc_batch(env):
    """DeviceBatch.run_crc_batch() == run() on a sha1=False batch; a batch with SHA-1 states raises."""
    from efes_amd.batch import DeviceBatch
    T = env["T"]
    lengths = [0, 1, 4097, T, 3 * T + 5, (1 << 20) + 3]
    offsets = [i * (2 << 20) + i for i in range(len(lengths))]
    crcs = np.array([0, 1, 0xFFFFFFFF, 7, 8, 9], dtype=np.uint32)
    a = DeviceBatch(env["buf"].data_ptr(), offsets, lengths, sha1=False, crcs=crcs, ctx=env["ctx"])
    b = DeviceBatch(env["buf"].data_ptr(), offsets, lengths, sha1=False, crcs=crcs, ctx=env["ctx"])
    a.run_crc_batch()
    b.run()
    assert (a.crc_sum() == b.crc_sum()).all() and (a.sums_host() == b.sums_host()).all()
    assert (a.status_host() == 0).all() and (b.status_host() == 0).all()
    assert a.crc_sum().tolist() == [zlib.crc32(env["host"][o:o + n], int(c)) for o, n, c in zip(offsets, lengths, crcs)]
    a.reset()
    a.run_crc_batch()  # the scratch is kept
    assert (a.crc_sum() == b.crc_sum()).all()
    with pytest.raises(ValueError):
        DeviceBatch(env["buf"].data_ptr(), offsets, lengths, ctx=env["ctx"]).run_crc_batch()
