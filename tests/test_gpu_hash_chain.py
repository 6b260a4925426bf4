"""GPU parity of the chained SHA-1 + CRC-32 call (efes_hash_chain): a job with EFES_JOB_CHAIN is the next
Write into the states of the job before it, and one wavefront walks each chain.  The yardstick is Go's
Write; Write; ... into one digest pair: every case replays each chain as successive write() calls on the
oracle's sha1digest and zlib.crc32 and compares status, the full 104-byte state (h, all 64 bytes of x, nx,
len), crc and every FINALIZE member's 24-byte sum; an invalid member keeps its sentinels.  hashlib is a
second check on the digests.  Unflagged arrays are compared byte for byte with EFES_MODE_DEEP.  Bit-exact."""
import hashlib
import random
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIN, INIT, SUM_ONLY, CHAIN = 0x1, 0x2, 0x4, 0x8
OK, STATE, ARG = 0, -2, -4
BUF_BYTES = 8 << 20


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from efes_amd import _lib, batch, hashing
    from oracle import oracle
    ctx = hashing.default_context(0)
    buf = torch.empty(BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    ctx.fill_synthetic(buf.data_ptr(), BUF_BYTES, 0x5A1C4A1, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(torch=torch, hashing=hashing, batch=batch, lib=_lib, ctx=ctx, oracle=oracle, buf=buf,
                host=buf.cpu().numpy())


def job(off, n, flags, sha, crc):
    """sha / crc: index of the SHA-1 / CRC state the job names (None: a NULL pointer)."""
    return dict(off=off, n=n, flags=flags, sha=sha, crc=crc)


def state_after(env, data: bytes, nx=None):
    """A SHA1_STATE_DTYPE row: the oracle's state after Write(data); nx = 64 is made from a 63-byte tail
    plus one more pending byte (no Write leaves it, a caller's state may hold it)."""
    s = env["oracle"].Sha1()
    assert s.write(data) == 0
    row = np.zeros(1, dtype=env["lib"].SHA1_STATE_DTYPE)[0]
    row["h"], row["x"], row["nx"], row["len"] = list(s.st.h), list(bytes(s.st.x)), s.st.nx, s.st.len
    if nx == 64:
        assert s.st.nx == 63
        row["x"][63], row["nx"], row["len"] = 0x3C, 64, s.st.len + 1
    elif nx is not None:
        assert s.st.nx == nx
    return row


def _oracle_of(env, row):
    s = env["oracle"].Sha1(reset=False)
    s.st.h[:] = [int(v) for v in row["h"]]
    s.st.x[:] = bytes(row["x"])
    s.st.nx, s.st.len = int(row["nx"]), int(row["len"])
    return s


def _row_of(env, s):
    row = np.zeros(1, dtype=env["lib"].SHA1_STATE_DTYPE)[0]
    row["h"], row["x"], row["nx"], row["len"] = list(s.st.h), list(bytes(s.st.x)), s.st.nx, s.st.len
    return row


def expectation(env, specs, states_in, crc_in):
    """(states, crcs, sums, status) after the chains' members as successive Writes: validity job by job per
    efes_hash.h, each valid member one write() on the oracle's digest and one zlib.crc32 step."""
    host = env["host"]
    states = np.array(states_in, dtype=env["lib"].SHA1_STATE_DTYPE)
    crcs = [int(c) for c in crc_in]
    sums = np.full((len(specs), 24), 0xA5, dtype=np.uint8)
    status = np.full(len(specs), -99, dtype=np.int32)
    bad, prev = False, None
    for j, s in enumerate(specs):
        if s["flags"] & CHAIN:
            bad = (bad or j == 0 or s["sha"] != prev["sha"] or s["crc"] != prev["crc"] or
                   (s["sha"] is None and s["crc"] is None) or bool(s["flags"] & (INIT | SUM_ONLY)) or
                   bool(prev["flags"] & SUM_ONLY))
        else:
            bad = False
        prev = s
        if bad:
            status[j] = ARG
            continue
        data = bytes(host[s["off"]:s["off"] + s["n"]])
        do_sha, do_crc = s["sha"] is not None, s["crc"] is not None
        d, crc = None, 0
        if do_sha:
            d = env["oracle"].Sha1() if s["flags"] & INIT else _oracle_of(env, states[s["sha"]])
            if d.write(data):  # Go panics in Write (sha1.go:62): nothing of this member is written
                status[j] = STATE
                continue
        if do_crc:
            crc = zlib.crc32(data, 0 if s["flags"] & INIT else crcs[s["crc"]])
        status[j] = OK
        if s["flags"] & FIN:
            dig = bytes(20)
            if do_sha:
                rc, dig = d.sum()
                if rc:  # d.nx != 0 in checkSum (sha1.go:107-109)
                    status[j], dig = STATE, bytes(20)
            sums[j] = np.frombuffer(dig + (crc.to_bytes(4, "big") if do_crc else bytes(4)), dtype=np.uint8)
        if not s["flags"] & SUM_ONLY:
            if do_sha:
                states[s["sha"]] = _row_of(env, d)
            if do_crc:
                crcs[s["crc"]] = crc
    return states, np.array(crcs, dtype=np.uint32), sums, status


class Chains:
    """A device job array over env's buffer with SHA-1 states states_in[], CRC states crc_in[] and sentinel
    sums / status."""

    def __init__(self, env, specs, states_in, crc_in):
        torch, lib = env["torch"], env["lib"]
        self.env, self.specs, self.n = env, specs, len(specs)
        self.states_in = np.array(states_in, dtype=lib.SHA1_STATE_DTYPE).reshape(-1)
        self.crc_in = np.array(crc_in, dtype=np.uint32).reshape(-1)
        n = max(self.n, 1)
        pad = np.zeros(1, dtype=lib.SHA1_STATE_DTYPE)
        self.states = torch.from_numpy(np.concatenate([self.states_in, pad]).view(np.uint8).copy()).to("cuda:0")
        self.crcs = torch.from_numpy(np.concatenate([self.crc_in, [0]]).astype(np.uint32).view(np.int32).copy()).to("cuda:0")
        self.sums = torch.full((n * 24,), 0xA5, dtype=torch.uint8, device="cuda:0")
        self.status = torch.full((n,), -99, dtype=torch.int32, device="cuda:0")
        idx = np.arange(self.n, dtype=np.uint64)
        rec = np.zeros(self.n, dtype=lib.JOB_DTYPE)
        rec["data"] = np.uint64(env["buf"].data_ptr()) + np.array([s["off"] for s in specs], dtype=np.uint64)
        rec["length"] = np.array([s["n"] for s in specs], dtype=np.uint64)
        rec["flags"] = np.array([s["flags"] for s in specs], dtype=np.uint32)
        rec["sha1"] = np.array([0 if s["sha"] is None else self.states.data_ptr() + 104 * s["sha"] for s in specs], dtype=np.uint64)
        rec["crc32"] = np.array([0 if s["crc"] is None else self.crcs.data_ptr() + 4 * s["crc"] for s in specs], dtype=np.uint64)
        rec["sum"] = np.uint64(self.sums.data_ptr()) + idx * np.uint64(24)
        rec["status"] = np.uint64(self.status.data_ptr()) + idx * np.uint64(4)
        self.rec = rec
        self.jobs = torch.from_numpy(rec.view(np.uint8).copy()).to("cuda:0") if self.n else torch.zeros(56, dtype=torch.uint8, device="cuda:0")
        self.scratch_bytes = env["hashing"].hash_chain_scratch(self.n)
        self.scratch = torch.empty(max(self.scratch_bytes, 16), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def run(self, stream="current", scratch=None, first=0, count=None):
        s = self.env["torch"].cuda.current_stream().cuda_stream if stream == "current" else stream
        scratch = self.scratch if scratch is None else scratch
        count = self.n - first if count is None else count
        self.env["ctx"].hash_chain(self.jobs.data_ptr() + 56 * first, count, scratch.data_ptr(), scratch.numel(), s)

    def run_deep(self):
        self.env["ctx"].submit(self.jobs.data_ptr(), self.n, self.env["torch"].cuda.current_stream().cuda_stream,
                               self.env["lib"].MODE_DEEP)

    def results(self):
        self.env["torch"].cuda.synchronize()
        lib = self.env["lib"]
        return (self.states.cpu().numpy().view(lib.SHA1_STATE_DTYPE)[:self.states_in.size].copy(),
                self.crcs.cpu().numpy().view(np.uint32)[:self.crc_in.size].copy(),
                self.sums.cpu().numpy()[:24 * self.n].reshape(self.n, 24).copy(), self.status.cpu().numpy()[:self.n].copy())

    def check(self, what=""):
        states, crcs, sums, status = self.results()
        estates, ecrcs, esums, estatus = expectation(self.env, self.specs, self.states_in, self.crc_in)
        bad = np.nonzero(status != estatus)[0]
        assert bad.size == 0, (what, "status", [(int(j), self.specs[j], int(status[j]), int(estatus[j])) for j in bad[:5]])
        bad = np.nonzero((sums != esums).any(axis=1))[0]
        assert bad.size == 0, (what, "sum", [(int(j), self.specs[j], bytes(sums[j]).hex(), bytes(esums[j]).hex()) for j in bad[:5]])
        for f in ("h", "x", "nx", "len"):  # _pad is ignored by the contract
            bad = np.nonzero((states[f] != estates[f]).reshape(states.size, -1).any(axis=1))[0]
            assert bad.size == 0, (what, "state", f, [(int(k), states[f][k].tolist(), estates[f][k].tolist()) for k in bad[:3]])
        bad = np.nonzero(crcs != ecrcs)[0]
        assert bad.size == 0, (what, "crc", [(int(k), hex(crcs[k]), hex(ecrcs[k])) for k in bad[:5]])
        return estates, ecrcs, esums, estatus


def _kinds(kind, k):
    """(sha index, crc index) of state k for a fused, SHA-1-only or CRC-only chain."""
    return (k if kind != "crc" else None, k if kind != "sha" else None)


@pytest.mark.parametrize("kind", ["fused", "sha", "crc"])
def test_unflagged_array_equals_deep(env, kind):
    """40 seeded jobs of 0-70 000 bytes at offsets 0-15 mod 16, INIT or resumed from mid-block states (nx in
    {1, 55, 63, 64}), with and without FINALIZE, one SUM_ONLY: states, crcs, sums and status byte-identical to
    efes_hash_submit_mode(EFES_MODE_DEEP) on copies of the same inputs, and equal to the oracle."""
    rng = random.Random({"fused": 40, "sha": 41, "crc": 42}[kind])
    host = env["host"]
    specs, states_in, crc_in = [], [], []
    for k in range(40):
        n = rng.choice([0, 1, 63, 64, 65, rng.randrange(0, 70001), rng.randrange(0, 70001)])
        off = 16 * rng.randrange(0, (BUF_BYTES - 70016) // 16) + (k % 16)
        sha, crc = _kinds(kind, k)
        flags = rng.choice([0, FIN])
        nx = [None, 1, 55, 63, 64][k % 5]
        if nx is None:
            flags |= INIT
            states_in.append(state_after(env, b""))
        else:
            pre = 64 * rng.randrange(0, 3) + (63 if nx == 64 else nx)
            states_in.append(state_after(env, bytes(host[k * 256:k * 256 + pre]), nx))
        crc_in.append(rng.getrandbits(32))
        if k == 17:  # Sum of the in-state on a copy
            n, flags = 0, FIN | SUM_ONLY
        specs.append(job(off, n, flags, sha, crc))
    A, B = Chains(env, specs, states_in, crc_in), Chains(env, specs, states_in, crc_in)
    A.run_deep()
    B.run()
    ra, rb = A.results(), B.results()
    for a, b, what in zip(ra, rb, ("state", "crc", "sum", "status")):
        assert a.tobytes() == b.tobytes(), (kind, what)
    B.check(kind)


BOUNDARY_LENGTHS = [0, 1, 55, 56, 63, 64, 65, 119, 128, 4095, 4097, 65539]


def _boundary_object(kind, flags_head):
    specs, off = [], 4096
    for i, n in enumerate(BOUNDARY_LENGTHS):
        off = (off + 15) // 16 * 16 + [0, 1, 3, 15][i % 4]
        sha, crc = _kinds(kind, 0)
        specs.append(job(off, n, (CHAIN if i else flags_head) | FIN, sha, crc))
        off += n
    return specs


@pytest.mark.parametrize("kind,start", [("fused", "init"), ("fused", "nx37"), ("sha", "init"), ("crc", "init")])
def test_block_boundaries_inside_a_chain(env, kind, start):
    """One object in extents of 0 ... 65 539 bytes at data offsets 0, 1, 3, 15 mod 16 in turn, the running
    digest after every extent, from INIT and from an in-state with nx = 37."""
    host = env["host"]
    pre = bytes(host[100:100 + 64 + 37]) if start == "nx37" else b""
    specs = _boundary_object(kind, INIT if start == "init" else 0)
    C = Chains(env, specs, [state_after(env, pre)], [zlib.crc32(pre)])
    C.run()
    _, _, esums, estatus = C.check((kind, start))
    assert (estatus == OK).all()
    h, crc = hashlib.sha1(pre), zlib.crc32(pre)
    for j, s in enumerate(specs):  # hashlib / zlib over the prefix: the second check
        data = bytes(host[s["off"]:s["off"] + s["n"]])
        h.update(data)
        crc = zlib.crc32(data, crc)
        want = (h.digest() if kind != "crc" else bytes(20)) + (crc.to_bytes(4, "big") if kind != "sha" else bytes(4))
        assert bytes(esums[j]) == want, (kind, start, j)


def _seeded_chains(rng, count, kinds=("fused", "sha", "crc")):
    """count jobs in chains of 1-5 members of 0-300 bytes (the last chain cut at count); state k is chain k's."""
    specs, k = [], 0
    while len(specs) < count:
        members = min(rng.randrange(1, 6), count - len(specs))
        sha, crc = _kinds(rng.choice(kinds), k)
        for i in range(members):
            n = rng.randrange(0, 301)
            flags = (CHAIN if i else rng.choice([0, INIT])) | rng.choice([0, FIN])
            specs.append(job(rng.randrange(0, BUF_BYTES - n), n, flags, sha, crc))
        k += 1
    return specs, k


def _seeded_states(env, rng, k):
    host = env["host"]
    rows = [state_after(env, bytes(host[i * 64:i * 64 + rng.randrange(0, 200)])) for i in range(k)]
    return rows, [rng.getrandbits(32) for _ in range(k)]


@pytest.mark.parametrize("count", [1, 1023, 1024, 1025, 2049])
def test_prep_boundaries(env, count):
    """Seeded chains of 1-5 members over job counts around the 1024-job blocks of the head count, chains
    that straddle the block borders among them."""
    rng = random.Random({1025: 1026}.get(count, count))  # seeds whose chains cross every border
    specs, k = _seeded_chains(rng, count)
    assert all(specs[b]["flags"] & CHAIN for b in range(1024, count, 1024)), "a chain straddles each block border"
    states_in, crc_in = _seeded_states(env, rng, k)
    C = Chains(env, specs, states_in, crc_in)
    C.run()
    C.check(count)


@pytest.mark.parametrize("shape", ["1100-members-of-7-bytes", "one-chain-of-2049"])
def test_long_chains_across_blocks(env, shape):
    """A chain of 1100 members of 7 bytes between chains of one, and an array that is one chain of 2049
    members: a chain may span blocks of the head count."""
    rng = random.Random(1100)
    if shape == "one-chain-of-2049":
        specs = [job(3 + 11 * i, rng.randrange(0, 40), (CHAIN if i else INIT) | (FIN if i % 7 == 0 or i == 2048 else 0), 0, 0)
                 for i in range(2049)]
        k = 1
    else:
        specs = [job(64 * i, 100, INIT | FIN, i, i) for i in range(30)]
        specs += [job(5000 + 7 * i, 7, (CHAIN if i else 0) | (FIN if i % 100 == 99 else 0), 30, 30) for i in range(1100)]
        specs += [job(64 * i + 1, 100, FIN, i, i) for i in range(31, 40)]
        k = 40
    states_in, crc_in = _seeded_states(env, rng, k)
    C = Chains(env, specs, states_in, crc_in)
    C.run()
    C.check(shape)


def test_more_chains_than_resident_waves(env):
    """20 000 fused chains of 2 members of 1-200 bytes: every wave draws several tickets.  All digests
    against hashlib and zlib."""
    torch, lib, host = env["torch"], env["lib"], env["host"]
    rng = np.random.default_rng(20000)
    nobj = 20000
    lens = rng.integers(1, 201, size=2 * nobj)
    offs = rng.integers(0, BUF_BYTES - 200, size=2 * nobj)
    objects = [[(int(offs[2 * i]), int(lens[2 * i])), (int(offs[2 * i + 1]), int(lens[2 * i + 1]))] for i in range(nobj)]
    O = env["batch"].DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, ctx=env["ctx"])
    O.run()
    assert (O.status_host() == OK).all()
    sha, crc = O.sha1_hex(), O.crc_sum()
    for i, ((a, n), (b, m)) in enumerate(objects):
        data = bytes(host[a:a + n]) + bytes(host[b:b + m])
        assert sha[i] == hashlib.sha1(data).hexdigest(), i
        assert int(crc[i]) == zlib.crc32(data), i
    st = O.states_host()
    assert (st["len"] == lens.reshape(nobj, 2).sum(axis=1)).all() and (st["nx"] == st["len"] % 64).all()


def _invalid_case(rule):
    """Four chains over states 0..3 (+4: another state); the rule's member sits at job 4, in the middle of
    chain 1 (jobs 2-7).  Returns the specs and the jobs that must get EFES_ERR_ARG."""
    def chain(k, members, head=INIT):
        return [job(1000 * k + 97 * i, 50 + 13 * i, (CHAIN if i else head) | FIN, k, k) for i in range(members)]
    specs = chain(0, 2) + chain(1, 6) + chain(2, 3) + chain(3, 1)
    bad = [4, 5, 6, 7]
    if rule == "flagged-job-0":
        specs[0]["flags"] |= CHAIN
        bad = [0, 1]
    elif rule == "other-sha1":
        specs[4]["sha"] = 4
    elif rule == "other-crc32":
        specs[4]["crc"] = 4
    elif rule == "both-null":
        specs[4]["sha"] = specs[4]["crc"] = None
    elif rule == "with-init":
        specs[4]["flags"] |= INIT
    elif rule == "with-sum-only":
        specs[4]["flags"] |= SUM_ONLY
        specs[4]["n"] = 0
    elif rule == "after-sum-only-head":
        specs[2]["flags"], specs[2]["n"] = FIN | SUM_ONLY, 0
        bad = [3, 4, 5, 6, 7]
    elif rule == "after-invalid-member":
        specs[4]["crc"] = 4  # invalid by itself; job 5 names the chain's states again and is valid by itself
    return specs, bad


@pytest.mark.parametrize("rule", ["flagged-job-0", "other-sha1", "other-crc32", "both-null", "with-init", "with-sum-only",
                                  "after-sum-only-head", "after-invalid-member"])
def test_invalid_members(env, rule):
    """One case per rule of efes_hash.h, between valid neighbours: EFES_ERR_ARG for the member and every
    member behind it, their sums untouched, the states as after the valid prefix, the other chains correct."""
    specs, bad = _invalid_case(rule)
    rng = random.Random(len(rule))
    states_in, crc_in = _seeded_states(env, rng, 5)
    C = Chains(env, specs, states_in, crc_in)
    C.run()
    _, _, esums, estatus = C.check(rule)
    assert [j for j in range(len(specs)) if estatus[j] == ARG] == bad, (rule, estatus)
    assert (esums[bad] == 0xA5).all()
    states, crcs, _, _ = C.results()
    assert states[4].tobytes() == C.states_in[4].tobytes() and crcs[4] == C.crc_in[4], "the other state was written"


def test_go_panic_states(env):
    """nx = 65 at a Write (sha1.go:62): every member gets EFES_ERR_STATE and the state is untouched.
    nx = -1: Write skips the pending block, Sum panics (sha1.go:107-109), the state is written."""
    host = env["host"]
    s65, sneg = state_after(env, bytes(host[:64 + 20])), state_after(env, bytes(host[:64 + 20]))
    s65["nx"], sneg["nx"] = 65, -1
    specs = [job(300 + 70 * i, 70, (CHAIN if i else 0) | FIN, 0, 0) for i in range(3)]
    specs += [job(900 + 128 * i, [128, 0, 64][i], (CHAIN if i else 0) | (FIN if i != 1 else 0), 1, 1) for i in range(3)]
    C = Chains(env, specs, [s65, sneg], [0x12345678, 0x9ABCDEF0])
    C.run()
    _, _, esums, estatus = C.check()
    assert estatus.tolist() == [STATE, STATE, STATE, STATE, OK, STATE]
    assert (esums[:3] == 0xA5).all()
    states, crcs, _, _ = C.results()
    assert states[0].tobytes() == s65.tobytes() and crcs[0] == 0x12345678


def test_composition(env):
    """An object in 6 extents as one call, as two calls of 3 + 3 (the second head unflagged, no INIT) and as
    one efes_hash_submit of the contiguous bytes: the same sums, crc and state."""
    host = env["host"]
    lens = [1000, 37, 64, 0, 4133, 91]
    offs = np.concatenate(([0], np.cumsum(lens)))[:-1] + 7777
    one = [job(int(o), n, (CHAIN if i else INIT) | FIN, 0, 0) for i, (o, n) in enumerate(zip(offs, lens))]
    two = [dict(s) for s in one]
    two[3]["flags"] = FIN
    whole = [job(7777, sum(lens), INIT | FIN, 0, 0)]
    fresh = [state_after(env, b"")]
    A, B, W = Chains(env, one, fresh, [0]), Chains(env, two, fresh, [0]), Chains(env, whole, fresh, [0])
    A.run()
    B.run(first=0, count=3)
    B.run(first=3, count=3)
    W.env["ctx"].submit(W.jobs.data_ptr(), 1, env["torch"].cuda.current_stream().cuda_stream)
    A.check("one call")
    ra, rb, rw = A.results(), B.results(), W.results()
    for a, b, what in zip(ra, rb, ("state", "crc", "sum", "status")):
        assert a.tobytes() == b.tobytes(), what
    data = bytes(host[7777:7777 + sum(lens)])
    assert bytes(ra[2][5]) == hashlib.sha1(data).digest() + zlib.crc32(data).to_bytes(4, "big") == bytes(rw[2][0])
    for f in ("h", "nx", "len"):
        assert ra[0][f].tolist() == rw[0][f].tolist(), f
    # x: the last extent's tail over the stale bytes of earlier Writes, where one Write of the whole leaves its own
    nx = int(ra[0]["nx"][0])
    assert bytes(ra[0]["x"][0][:nx]) == bytes(rw[0]["x"][0][:nx]) == data[len(data) - nx:]
    assert ra[1][0] == rw[1][0]


def test_streams_and_scratch_reuse(env):
    """Two calls on two streams with a scratch each; then three calls back to back on one stream sharing
    one scratch, with 5, 900 and 3 chains: the count and the ticket are re-initialised by every call."""
    torch = env["torch"]
    rng = random.Random(77)

    def make(chains):
        specs = []
        for k in range(chains):
            for i in range(rng.randrange(1, 4)):
                n = rng.randrange(0, 500)
                specs.append(job(rng.randrange(0, BUF_BYTES - n), n, (CHAIN if i else INIT) | FIN, k, k))
        states_in, crc_in = _seeded_states(env, rng, chains)
        return Chains(env, specs, states_in, crc_in)

    A, B = make(300), make(200)
    sa, sb = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    A.run(sa.cuda_stream)
    B.run(sb.cuda_stream)
    A.check("stream a")
    B.check("stream b")
    sets = [make(5), make(900), make(3)]
    shared = torch.empty(max(c.scratch_bytes for c in sets), dtype=torch.uint8, device="cuda:0")
    for c in sets:
        c.run(sa.cuda_stream, scratch=shared)
    for c, what in zip(sets, (5, 900, 3)):
        c.check(what)


def test_arguments(env):
    torch, lib, ctx = env["torch"], env["lib"], env["ctx"]
    L = lib.lib()
    C = Chains(env, [job(0, 100, INIT | FIN, 0, 0), job(100, 100, CHAIN | FIN, 0, 0)], [state_after(env, b"")], [0])
    j, s, nb = C.jobs.data_ptr(), C.scratch.data_ptr(), C.scratch_bytes
    assert s % 16 == 0
    assert L.efes_hash_chain(ctx.handle, None, 0, None, 0, None) == lib.EFES_OK
    assert L.efes_hash_chain(ctx.handle, j, 0, s, nb, None) == lib.EFES_OK
    assert L.efes_hash_chain(ctx.handle, None, 2, s, nb, None) == lib.EFES_ERR_ARG
    assert L.efes_hash_chain(ctx.handle, j, 2, None, nb, None) == lib.EFES_ERR_ARG
    big = torch.empty(nb + 16, dtype=torch.uint8, device="cuda:0")
    assert L.efes_hash_chain(ctx.handle, j, 2, big.data_ptr() + 8, nb, None) == lib.EFES_ERR_ARG
    assert L.efes_hash_chain(ctx.handle, j, 2, s, nb - 1, None) == lib.EFES_ERR_ARG
    assert L.efes_hash_chain(ctx.handle, j, lib.EFES_HASH_CHAIN_MAX_JOBS + 1, s, 1 << 40, None) == lib.EFES_ERR_ARG
    torch.cuda.synchronize()
    assert (C.status.cpu().numpy() == -99).all(), "a refused call launched"
    C.run()
    C.check()


def test_device_objects_sha1(env, monkeypatch):
    """DeviceObjects(sha1=True): objects of 0, 1 and 9 extents, running digests; the default-argument object
    still goes through efes_crc32_chain."""
    host, batch = env["host"], env["batch"]
    ext9 = [(20000 + 1031 * i, [0, 1, 63, 64, 65, 700, 4096, 5, 129][i]) for i in range(9)]
    objects = [[], [(100, 777)], ext9]
    O = batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, running=True, ctx=env["ctx"])
    O.run()
    assert (O.status_host() == OK).all() and O.status_host().size == 10
    cat = [b"".join(bytes(host[a:a + n]) for a, n in o) for o in objects]
    assert O.sha1_hex() == [None] + [hashlib.sha1(c).hexdigest() for c in cat[1:]]
    assert O.crc_sum().tolist() == [0] + [zlib.crc32(c) for c in cat[1:]]
    run_sha, run_crc, h, crc = [], [], hashlib.sha1(), 0
    d = env["oracle"].Sha1()
    for a, n in ext9:
        h.update(bytes(host[a:a + n]))
        crc = zlib.crc32(bytes(host[a:a + n]), crc)
        assert d.write(bytes(host[a:a + n])) == 0
        run_sha.append(h.hexdigest())
        run_crc.append(crc)
    assert O.running_sha1() == [hashlib.sha1(cat[1]).hexdigest()] + run_sha
    assert O.running_crcs().tolist() == [zlib.crc32(cat[1])] + run_crc
    st = O.states_host()
    assert st.size == 3
    assert st[0].tobytes() == batch.fresh_states(1)[0].tobytes()  # no extents: no job, the in-state kept
    assert st[2]["h"].tolist() == list(d.st.h) and bytes(st[2]["x"]) == bytes(d.st.x)
    assert int(st[2]["nx"]) == d.st.nx and int(st[2]["len"]) == d.st.len
    # the default object: CRC only, through efes_crc32_chain
    calls = []
    ctx = env["ctx"]
    orig_crc, orig_hash = type(ctx).crc32_chain, type(ctx).hash_chain
    monkeypatch.setattr(type(ctx), "crc32_chain", lambda self, *a: calls.append("crc32_chain") or orig_crc(self, *a))
    monkeypatch.setattr(type(ctx), "hash_chain", lambda self, *a: calls.append("hash_chain") or orig_hash(self, *a))
    D = batch.DeviceObjects(env["buf"].data_ptr(), objects, ctx=ctx)
    D.run()
    assert calls == ["crc32_chain"]
    assert D.crc_sum().tolist() == [0] + [zlib.crc32(c) for c in cat[1:]]
    with pytest.raises(ValueError):
        D.sha1_hex()
