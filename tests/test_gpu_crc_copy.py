"""GPU parity of copy with CRC (efes_crc32_copy): efes_crc32_chain plus a copy of each job's bytes to dst[j]
in the same pass.  Every case runs the copy call and, on a second job array over fresh copies of the
states, efes_crc32_chain: states, sums, statuses and the SHA-1 sentinels must be bit-equal.  The destination
buffer is pre-filled with a sentinel byte and compared WHOLE against an image built on the host: the source
bytes in the range of every valid job that has a destination, the sentinel everywhere else -- the guard
bytes (at least 64 on either side of every range) and the ranges of jobs that are not copied (dst[j] ==
NULL, sha1 != NULL, crc32 == NULL).  Only the ranges of chain members that are invalid for another reason
are left out: the header leaves them unspecified.  Last, zlib over the destination bytes read back must
give the states the call left: that ties the copy to the check."""
import random
import zlib

import numpy as np
import pytest

from test_gpu_crc_chain import ARG, BUF_BYTES, CHAIN, FIN, INIT, SUM_ONLY, Chains, _invalid_cases, job

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE
GUARD = 64
DST_BYTES = 40 << 20
MIB = 1 << 20


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from efes_amd import _lib, hashing
    ctx = hashing.default_context(0)
    buf = torch.empty(BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(DST_BYTES, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ctx.fill_synthetic(buf.data_ptr(), BUF_BYTES, 0xC09F, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(torch=torch, hashing=hashing, lib=_lib, ctx=ctx, buf=buf, dst=dst, host=buf.cpu().numpy(),
                T=_lib.EFES_CRC_BATCH_TILE)


class Layout:
    """Destination ranges handed out front to back: at least GUARD bytes between any two and at either end
    of the buffer, each starting at the asked offset mod 16."""

    def __init__(self, start=0):
        self.at = start

    def place(self, n, mod16=0):
        start = (self.at + GUARD + 15) // 16 * 16 + mod16
        self.at = start + n
        assert self.at + GUARD <= DST_BYTES
        return start


class Copy:
    """specs: the jobs (job() of the chain tests); dsts: per job the offset of its destination range in
    env's destination buffer, or None for dst[j] == NULL."""

    def __init__(self, env, specs, crc_in, dsts, src_host=None):
        torch = env["torch"]
        assert len(dsts) == len(specs)
        self.env, self.specs, self.dsts = env, specs, dsts
        self.src_host = env["host"] if src_host is None else src_host
        self.copy, self.chain = Chains(env, specs, crc_in), Chains(env, specs, crc_in)
        base = env["dst"].data_ptr()
        ptr = np.array([0 if d is None else base + d for d in dsts] + [0], dtype=np.uint64)
        self.ptrs = torch.from_numpy(ptr.view(np.int64).copy()).to("cuda:0")
        self.scratch_bytes = env["hashing"].crc32_copy_scratch(len(specs))
        self.scratch = torch.empty(max(self.scratch_bytes, 16), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def submit(self, scratch=None):
        scratch = self.scratch if scratch is None else scratch
        s = self.env["torch"].cuda.current_stream().cuda_stream
        self.env["ctx"].crc32_copy(self.copy.jobs.data_ptr(), self.ptrs.data_ptr(), self.copy.n, scratch.data_ptr(),
                                   self.scratch_bytes, s)

    def run(self):
        self.env["dst"].fill_(SENTINEL)
        self.submit()
        self.chain.run()

    def uncopied(self, j):
        s = self.specs[j]
        return self.dsts[j] is None or s["sha1"] or s["state"] is None

    def same_as_chain(self, what=""):
        """Everything efes_crc32_chain writes, bit for bit; returns the copy call's results."""
        got, ref = self.copy.results(), self.chain.results()
        for a, b, name in zip(got, ref, ("state", "sum", "status", "sha1")):
            assert a.shape == b.shape and (a == b).all(), (what, name, np.nonzero(a != b)[0][:5])
        return got

    def check(self, what=""):
        """Returns (statuses, the destination buffer on the host)."""
        crcs, _, status, _ = self.same_as_chain(what)
        img = self.env["dst"].cpu().numpy()
        want = np.full(DST_BYTES, SENTINEL, dtype=np.uint8)
        compare = np.ones(DST_BYTES, dtype=bool)
        for j, (s, d) in enumerate(zip(self.specs, self.dsts)):
            if self.uncopied(j):
                continue
            if status[j] == 0:
                want[d:d + s["n"]] = self.src_host[s["off"]:s["off"] + s["n"]]
            else:
                compare[d:d + s["n"]] = False  # unspecified: the old bytes or the source bytes
        bad = np.nonzero((img != want) & compare)[0]
        assert bad.size == 0, (what, "destination", bad[:8].tolist(), img[bad[:8]].tolist(), want[bad[:8]].tolist(),
                               [j for j, d in enumerate(self.dsts) if d is not None and d - GUARD <= bad[0] < d + self.specs[j]["n"] + GUARD])
        # zlib over what was landed (the source where a job has no destination) gives the states
        run = dict(enumerate(self.copy.crc_in))
        for j, s in enumerate(self.specs):
            if status[j] == 0 and s["state"] is not None and not s["flags"] & SUM_ONLY:
                data = self.src_host[s["off"]:s["off"] + s["n"]] if self.dsts[j] is None else img[self.dsts[j]:self.dsts[j] + s["n"]]
                run[s["state"]] = zlib.crc32(data, 0 if s["flags"] & INIT else run[s["state"]])
        assert [int(c) for c in crcs] == [run[k] for k in range(len(crcs))], (what, "zlib of the destination")
        return status, img


MATRIX_LENGTHS = [0, 1, 15, 16, 17, 33, 4095, 65535, 65536, 65537, 131072 + 5, 196608 + 16 * 63 + 9]


def test_alignment_matrix(env):
    """256 jobs in one call: source offset mod 16 = a and destination offset mod 16 = b for all (a, b), the
    lengths cycling through a head only, head + rest without a piece, one partial tile, exactly one tile,
    one tile + one piece, a whole-tile run plus a partial last tile, and three tiles."""
    rng = random.Random(256)
    pairs = [(a, b) for a in range(16) for b in range(16)]
    rng.shuffle(pairs)  # in job order the 12 lengths would meet only four values of b each
    lay, specs, dsts = Layout(), [], []
    for a, b in pairs:
        n = MATRIX_LENGTHS[len(specs) % len(MATRIX_LENGTHS)]
        specs.append(job(16 * rng.randrange(0, (BUF_BYTES - n - 16) // 16) + a, n, rng.choice([0, INIT]) | rng.choice([0, FIN]), len(specs)))
        dsts.append(lay.place(n, b))
    assert len(specs) == 256 and {(s["off"] % 16, d % 16) for s, d in zip(specs, dsts)} == set(pairs)
    for n in MATRIX_LENGTHS:  # every length meets at least 21 pairs, with odd and even, equal and unequal misalignments
        met = {(s["off"] % 16, d % 16) for s, d in zip(specs, dsts) if s["n"] == n}
        assert len(met) >= 21 and len({a for a, _ in met}) >= 8 and len({b for _, b in met}) >= 8 and len({(a - b) % 16 for a, b in met}) >= 8, (n, met)
    C = Copy(env, specs, [rng.getrandbits(32) for _ in specs], dsts)
    C.run()
    status, _ = C.check()
    assert (status == 0).all()


def test_workgroups_that_span_jobs(env):
    """40 unflagged jobs of 0..1.5 MiB, 28.6 MiB in all: more than 256 tiles, so a workgroup takes two or more
    consecutive tiles and its range crosses job boundaries.  Mixed alignments."""
    rng = random.Random(40)
    lengths = [rng.randrange(0, 3 * MIB // 2) for _ in range(40)]
    lengths[7] = 0
    total = sum(lengths)
    assert 20 * MIB <= total <= 30 * MIB and sum((n + env["T"] - 1) // env["T"] for n in lengths) > 256
    lay, specs, dsts = Layout(), [], []
    for k, n in enumerate(lengths):
        specs.append(job(rng.randrange(0, BUF_BYTES - n), n, rng.choice([0, INIT, FIN]), k))
        dsts.append(lay.place(n, rng.randrange(16)))
    C = Copy(env, specs, [rng.getrandbits(32) for _ in specs], dsts)
    C.run()
    status, _ = C.check()
    assert (status == 0).all()


def test_two_prefix_blocks(env):
    """2 500 jobs of 0-300 bytes with a 70 000-byte job every 97th: three blocks of the prefix sum, so the
    carry launch runs, and most jobs have no tile at all (the map pass lands them alone)."""
    rng = random.Random(2500)
    lay, specs, dsts, crc_in = Layout(), [], [], []
    for k in range(2500):
        n = 70000 if k % 97 == 96 else rng.randrange(0, 301)
        chained = k % 5 in (1, 2) and k > 0
        if not chained:
            crc_in.append(rng.getrandbits(32))
        specs.append(job(rng.randrange(0, BUF_BYTES - n), n, (CHAIN if chained else rng.choice([0, INIT])) | rng.choice([0, FIN]), len(crc_in) - 1))
        dsts.append(lay.place(n, rng.randrange(16)))
    C = Copy(env, specs, crc_in, dsts)
    C.run()
    status, _ = C.check()
    assert (status == 0).all()


def test_gather(env):
    """Three objects as chains with running sums, the destinations packed at byte granularity (the second
    object starts at an odd address): the destination is the concatenation and every running CRC is zlib
    over the destination prefix of its object."""
    T, host = env["T"], env["host"]
    rng = random.Random(3)
    objects = [[MIB + 77, 0, 5, 65536, 300000, 33], [17, 4096, 3 * T + 11, 1, 0], [0, 200001, 15, 16, 70000, 2 * T]]
    base = Layout().place(0, 0)
    specs, dsts, at, starts = [], [], base, []
    for k, ext in enumerate(objects):
        starts.append(at)
        for i, n in enumerate(ext):
            specs.append(job(rng.randrange(0, BUF_BYTES - n), n, FIN | (CHAIN if i else INIT), k))
            dsts.append(at)
            at += n
    assert starts[1] % 2 == 1 and at + GUARD <= DST_BYTES
    C = Copy(env, specs, [0x11111111, 0x22222222, 0x33333333], dsts)
    C.run()
    status, img = C.check()
    assert (status == 0).all()
    whole = b"".join(host[s["off"]:s["off"] + s["n"]].tobytes() for s in specs)
    assert img[base:at].tobytes() == whole
    sums = C.copy.results()[1]
    for j, (s, d) in enumerate(zip(specs, dsts)):
        prefix = zlib.crc32(img[starts[s["state"]]:d + s["n"]])
        assert bytes(sums[j]) == bytes(20) + prefix.to_bytes(4, "big"), j


def test_mixed_null_destinations(env):
    """Every third dst[j] is NULL: those jobs are hashed (the states say so) and nothing is written for them."""
    rng = random.Random(33)
    lay, specs, dsts, crc_in = Layout(), [], [], []
    for k in range(60):
        n = rng.choice([0, 9, 16, 300, 4097, 65536, 70001, rng.randrange(0, 400000)])
        chained = k % 4 in (1, 2)
        if not chained:
            crc_in.append(rng.getrandbits(32))
        specs.append(job(rng.randrange(0, BUF_BYTES - n), n, (CHAIN if chained else rng.choice([0, INIT])) | rng.choice([0, FIN]), len(crc_in) - 1))
        d = lay.place(n, rng.randrange(16))  # the area stays reserved, and must stay untouched
        dsts.append(None if k % 3 == 2 else d)
    C = Copy(env, specs, crc_in, dsts)
    C.run()
    status, _ = C.check()
    assert (status == 0).all()


@pytest.mark.parametrize("case", list(_invalid_cases()))
def test_invalid_members(env, case):
    """The chain call's invalid cases: statuses as the chain call gives them; a job with sha1 != NULL or
    crc32 == NULL leaves its destination all sentinel; for the other invalid members only the guards are
    asserted; the valid members before them and the chains before and behind are exact."""
    members, statuses = _invalid_cases()[case]
    rng = random.Random(case)
    lay = Layout()

    def place(parts):
        out = []
        for p in parts:
            n = 0 if p["flags"] & SUM_ONLY else rng.choice([7, 500, 70001, 2 * env["T"] + 21])
            out.append((job(rng.randrange(0, BUF_BYTES - n), n, p["flags"], p["state"], sha1=p.get("sha1", False)),
                        lay.place(n, rng.randrange(16))))
        return out
    before = place([dict(flags=INIT | FIN, state=0), dict(flags=CHAIN, state=0), dict(flags=CHAIN | FIN, state=0)])
    mid = place(members)
    after = place([dict(flags=FIN, state=3), dict(flags=CHAIN | FIN, state=3), dict(flags=CHAIN, state=3)])
    if case == "chain-on-job-0":
        before = []
    jobs = before + mid + after
    C = Copy(env, [s for s, _ in jobs], [rng.getrandbits(32) for _ in range(4)], [d for _, d in jobs])
    C.run()
    status, img = C.check(case)
    assert status.tolist() == [0] * len(before) + statuses + [0] * 3
    for (s, d), st in zip(mid, statuses):
        if s["sha1"] or s["state"] is None:
            assert st == ARG and s["n"] > 0 and (img[d:d + s["n"]] == SENTINEL).all()


def test_stream_order(env):
    """Two calls on one stream share one scratch, and the second call's sources are the first call's
    destinations: the final bytes are the original ones and both calls leave the same CRCs."""
    torch, host = env["torch"], env["host"]
    rng = random.Random(2)
    lay, specs, first, second, crc_in = Layout(), [], [], [], []
    for k in range(48):
        n = rng.choice([0, 1, 31, 5000, 65536, 65537, rng.randrange(0, 300000)])
        chained = k % 3 == 1
        if not chained:
            crc_in.append(rng.getrandbits(32))
        specs.append(job(rng.randrange(0, BUF_BYTES - n), n, (CHAIN if chained else 0) | FIN, len(crc_in) - 1))
        first.append(lay.place(n, rng.randrange(16)))
    for s in specs:
        second.append(lay.place(s["n"], rng.randrange(16)))
    A, B = Copy(env, specs, crc_in, first), Copy(env, specs, crc_in, second)
    rec = B.copy.jobs.cpu().numpy().view(env["lib"].JOB_DTYPE).copy()
    rec["data"] = np.uint64(env["dst"].data_ptr()) + np.array(first, dtype=np.uint64)  # read what the first call lands
    B.copy.jobs.copy_(torch.from_numpy(rec.view(np.uint8)))
    torch.cuda.synchronize()
    env["dst"].fill_(SENTINEL)
    A.submit()
    B.submit(A.scratch)
    A.chain.run()
    _, _, status, _ = A.same_as_chain("first call")
    assert (status == 0).all()
    img = env["dst"].cpu().numpy()
    for s, d1, d2 in zip(specs, first, second):
        want = host[s["off"]:s["off"] + s["n"]]
        assert (img[d1:d1 + s["n"]] == want).all() and (img[d2:d2 + s["n"]] == want).all(), s
    for a, b, name in zip(A.copy.results(), B.copy.results(), ("state", "sum", "status", "sha1")):
        assert (a == b).all(), name
    # nothing else was written: the ranges of both calls are all that differs from the sentinel
    touched = np.zeros(DST_BYTES, dtype=bool)
    for s, d1, d2 in zip(specs, first, second):
        touched[d1:d1 + s["n"]] = touched[d2:d2 + s["n"]] = True
    assert (img[~touched] == SENTINEL).all()


def test_device_objects_copy_to(env):
    """DeviceObjects(copy_to=...): the default layout (objects back to back, starts rounded up to 256) and
    explicit odd offsets; the destination holds each object's extents one behind the other."""
    from efes_amd.batch import DeviceObjects, default_copy_offsets
    T, host = env["T"], env["host"]
    rng = random.Random(29)
    objects = [[(rng.randrange(0, 1 << 24), rng.choice([0, 1, 4097, T, 3 * T + 5, rng.randrange(0, 1 << 19)])) for _ in range(k)]
               for k in (1, 9, 0, 17, 2)]
    whole = [b"".join(host[off:off + n].tobytes() for off, n in ext) for ext in objects]
    base = 4096 + 16
    odd, at = [], 1
    for w in whole:
        odd.append(at)
        at += len(w) + len(w) % 2 + GUARD  # every start odd
    for offsets in (None, odd):
        env["dst"].fill_(SENTINEL)
        d = DeviceObjects(env["buf"].data_ptr(), objects, running=True, ctx=env["ctx"], copy_to=env["dst"].data_ptr() + base,
                          copy_offsets=offsets)
        if offsets is None:
            want_off, want_room = default_copy_offsets(objects)
            assert d.copy_offsets.tolist() == want_off.tolist() and d.copy_bytes == want_room
            assert (d.copy_offsets % 256 == 0).all()
        else:
            assert d.copy_offsets.tolist() == odd and d.copy_bytes == odd[-1] + len(whole[-1])
        assert base + d.copy_bytes + GUARD <= DST_BYTES
        d.run()
        assert (d.status_host() == 0).all()
        assert d.crc_sum().tolist() == [zlib.crc32(w) for w in whole]
        img = env["dst"].cpu().numpy()
        want = np.full(DST_BYTES, SENTINEL, dtype=np.uint8)
        for w, o in zip(whole, d.copy_offsets.tolist()):
            want[base + o:base + o + len(w)] = np.frombuffer(w, dtype=np.uint8)
        assert (img == want).all(), np.nonzero(img != want)[0][:8]
        ref = DeviceObjects(env["buf"].data_ptr(), objects, running=True, ctx=env["ctx"])
        ref.run()
        assert d.running_crcs().tolist() == ref.running_crcs().tolist()


def test_arguments(env):
    """On a live context: a scratch that is too small or misaligned, njobs above the maximum and a NULL
    pointer array are EFES_ERR_ARG and write nothing; njobs == 0 is EFES_OK and launches nothing."""
    torch, lib = env["torch"], env["lib"]
    L, ctx = lib.lib(), env["ctx"]
    lay = Layout()
    specs = [job(3, 70000, FIN, 0), job(80000, 24, CHAIN | FIN, 0)]
    C = Copy(env, specs, [0xDEADBEEF], [lay.place(70000, 5), lay.place(24, 9)])
    s = torch.cuda.current_stream().cuda_stream
    jp, dp, sp, sb = C.copy.jobs.data_ptr(), C.ptrs.data_ptr(), C.scratch.data_ptr(), C.scratch_bytes
    big = torch.empty(sb + 64, dtype=torch.uint8, device="cuda:0")
    env["dst"].fill_(SENTINEL)
    assert L.efes_crc32_copy(ctx.handle, jp, dp, 0, sp, sb, s) == lib.EFES_OK
    assert L.efes_crc32_copy(ctx.handle, None, None, 0, None, 0, s) == lib.EFES_OK
    for args in [(jp, dp, lib.EFES_CRC_BATCH_MAX_JOBS + 1, sp, sb), (jp, dp, 2, None, sb), (jp, dp, 2, sp, sb - 1),
                 (jp, dp, 2, big.data_ptr() + 8, sb + 56), (jp, None, 2, sp, sb), (None, dp, 2, sp, sb)]:
        assert L.efes_crc32_copy(ctx.handle, *args, s) == lib.EFES_ERR_ARG, args
    torch.cuda.synchronize()
    crcs, sums, status, _ = C.copy.results()
    assert int(crcs[0]) == 0xDEADBEEF and (sums == 0xA5).all() and (status == -99).all()
    assert bool((env["dst"] == SENTINEL).all())
    C.run()
    status, _ = C.check()
    assert (status == 0).all()
