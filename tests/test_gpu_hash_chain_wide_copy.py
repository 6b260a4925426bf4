"""GPU parity of the wide chain walk with copy (efes_hash_chain_wide_copy): efes_hash_chain_wide plus a copy of
every member whose Write takes effect to dst[j], from the registers it is hashed from.  Every case runs the copy
call on one job array and efes_hash_chain_wide on a second one over fresh copies of the states: states, sums,
statuses (and records, where asked) must be the same bytes, and equal the oracle's replay of the chains as
successive Writes.  The destination buffer is pre-filled with a sentinel byte and compared WHOLE against an
image built on the host: the source bytes in the range of every member that is due a copy, the sentinel
everywhere else -- the guard bytes (at least 64 on either side of every range, except where a gathered object's
members abut on purpose) and the ranges of members that are not copied (dst[j] == NULL, EFES_ERR_ARG, a
panicking Write and the members behind it, a job that names no state, EFES_JOB_SUM_ONLY).  Which members are due
is worked out from the oracle's expectation, not from what the call left.  Bit-exact."""
import hashlib
import random
import zlib

import numpy as np
import pytest

from test_gpu_hash_chain import (ARG, BUF_BYTES, CHAIN, FIN, INIT, OK, STATE, SUM_ONLY, Chains, _kinds, _seeded_states,
                                 expectation, job, state_after)
from test_gpu_hash_chain_ckpt import CkptChains
from test_gpu_hash_chain_group import same_bytes
from test_gpu_hash_chain_wide import _invalid_wave, _ragged, _state_wave, run_wide

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE
GUARD = 64


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


class Layout:
    """Destination ranges handed out front to back (the Layout of the copy-with-CRC tests): at least GUARD
    bytes in front of every range placed and behind the last one, each starting at the asked offset mod 16;
    abut() puts a range right behind the one before it, as the members of a gathered object lie."""

    def __init__(self):
        self.at = 0

    def place(self, n, mod16=0):
        start = (self.at + GUARD + 15) // 16 * 16 + mod16
        self.at = start + n
        return start

    def abut(self, n):
        start = self.at
        self.at += n
        return start

    @property
    def size(self):
        return self.at + GUARD + 16


def _offset(rng, n, mis=None):
    mis = rng.randrange(0, 16) if mis is None else mis
    return 16 * rng.randrange(0, (BUF_BYTES - n - 16) // 16) + mis


def due_copies(env, specs, states_in, crc_in):
    """Per job: is its Write one that takes effect, so that it is copied?  From the oracle's expectation: status
    EFES_OK, or EFES_ERR_STATE with the sum written (raised at the Sum, sha1.go:107-109; a Write that panics
    leaves the sum's sentinel); never a job that names no state or an EFES_JOB_SUM_ONLY job."""
    _, _, esums, estatus = expectation(env, specs, states_in, crc_in)
    due = np.zeros(len(specs), dtype=bool)
    for j, s in enumerate(specs):
        took = estatus[j] == OK or (estatus[j] == STATE and not (esums[j] == 0xA5).all())
        due[j] = bool(took) and not (s["sha"] is None and s["crc"] is None) and not s["flags"] & SUM_ONLY
    return due, estatus


class Gather:
    """specs, states_in, crc_in as for Chains; dsts: per job the offset of its range in a destination buffer of
    `size` bytes, or None for dst[j] == NULL.  ckpt: keep record slots and pass them (CkptChains)."""

    def __init__(self, env, specs, states_in, crc_in, dsts, size, ckpt=False):
        torch = env["torch"]
        assert len(dsts) == len(specs)
        self.env, self.specs, self.dsts, self.size, self.ckpt = env, specs, dsts, size, ckpt
        cls = CkptChains if ckpt else Chains
        self.A, self.B = cls(env, specs, states_in, crc_in), cls(env, specs, states_in, crc_in)
        self.dst = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        base = self.dst.data_ptr()
        ptr = np.array([0 if d is None else base + d for d in dsts] + [0], dtype=np.uint64)
        self.ptrs = torch.from_numpy(ptr.view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()

    def submit(self, stream="current", with_ckpt=None):
        s = self.env["torch"].cuda.current_stream().cuda_stream if stream == "current" else stream
        with_ckpt = self.ckpt if with_ckpt is None else with_ckpt
        ck = self.A.ptrs.data_ptr() if with_ckpt else None
        self.env["ctx"].hash_chain_wide_copy(self.A.jobs.data_ptr(), self.A.n, self.ptrs.data_ptr(), ck,
                                             self.A.scratch.data_ptr(), self.A.scratch.numel(), s)

    def run(self, with_ckpt=None):
        with_ckpt = self.ckpt if with_ckpt is None else with_ckpt
        self.submit(with_ckpt=with_ckpt)
        run_wide(self.B, ckpt=self.B.ptrs.data_ptr() if with_ckpt else None)

    def image(self, due):
        """The destination as it must be: the sentinel, and the source bytes of every due member that has a range."""
        host = self.env["host"]
        want = np.full(self.size, SENTINEL, dtype=np.uint8)
        for j, (s, d) in enumerate(zip(self.specs, self.dsts)):
            if d is not None and due[j]:
                want[d:d + s["n"]] = host[s["off"]:s["off"] + s["n"]]
        return want

    def check(self, what="", oracle=True):
        """The common checks; returns (due, statuses expected, the destination on the host)."""
        if oracle:
            self.A.check(what)
        same_bytes(self.A, self.B, what)
        if self.ckpt:
            assert self.A.records().tobytes() == self.B.records().tobytes(), (what, "records")
        due, estatus = due_copies(self.env, self.specs, self.A.states_in, self.A.crc_in)
        img = self.dst.cpu().numpy()
        want = self.image(due)
        bad = np.nonzero(img != want)[0]
        assert bad.size == 0, (what, "destination", bad[:8].tolist(), img[bad[:8]].tolist(), want[bad[:8]].tolist(),
                               [(j, self.specs[j], bool(due[j])) for j, d in enumerate(self.dsts)
                                if d is not None and d - GUARD <= bad[0] < d + self.specs[j]["n"] + GUARD][:4])
        return due, estatus, img


# ---- 1. alignment matrix
MATRIX_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 5 * 64 + 63, 7 * 64, 24 * 64 + 1]


MATRIX_PAIRS = [(b, n) for b in (0, 1, 7, 8, 15) for n in MATRIX_LENGTHS]


@pytest.mark.parametrize("part", [0, 1])
@pytest.mark.parametrize("src16", [0, 1, 8, 15])
@pytest.mark.parametrize("kind", ["fused", "sha", "crc"])
def test_alignment_matrix(env, kind, src16, part):
    """One wave plus a lane, 65 chains of one member from INIT, every source at src16 mod 16 (0: the wave takes
    the 16-byte-aligned loads; else the funnel-shifted ones): the destination at 0, 1, 7, 8 and 15 mod 16 x the 14
    lengths (no block, blocks with and without a tail, 24 blocks + 1) are 70 pairs, shuffled once so that every
    round mixes short and long lanes, and dealt to two calls of 65, the second wrapping around."""
    order = list(MATRIX_PAIRS)
    random.Random(1100 + src16).shuffle(order)
    assert len(order) == 70 and {order[(65 * q + k) % 70] for q in (0, 1) for k in range(65)} == set(MATRIX_PAIRS)
    rng = random.Random(1100 + 16 * part + src16)
    lay, specs, dsts = Layout(), [], []
    for k in range(65):
        b, n = order[(65 * part + k) % 70]
        sha, crc = _kinds(kind, k)
        specs.append(job(_offset(rng, n, src16), n, INIT | FIN, sha, crc))
        dsts.append(lay.place(n, b))
        assert specs[-1]["off"] % 16 == src16 and dsts[-1] % 16 == b
    states_in, crc_in = _seeded_states(env, rng, 65)
    G = Gather(env, specs, states_in, crc_in, dsts, lay.size)
    assert G.dst.data_ptr() % 16 == 0 and env["buf"].data_ptr() % 16 == 0
    G.run()
    due, estatus, _ = G.check((kind, src16, part))
    assert due.all() and (estatus == OK).all()


# ---- 2. the uniform phase of the bulk loop
@pytest.mark.parametrize("case", ["aligned", "misaligned", "every-fifth-null"])
def test_uniform_phase(env, case):
    """64 chains x 3 members of 12-20 blocks with every lane live (the shape of the wide walk's own
    test_uniform_phase), each chain gathered contiguously.  Aligned: whole blocks at 16-byte aligned sources and
    destinations; misaligned: sources at 1-15 mod 16, lengths with tails, destinations at seeded alignments.  In
    the third run every fifth dst[j] is NULL: those ranges keep the sentinel and the digests do not change."""
    aligned = case == "aligned"
    rng = random.Random(1200 + len(case))
    lay, specs, dsts = Layout(), [], []
    for k in range(64):
        sha, crc = _kinds(["fused", "fused", "sha", "crc"][k % 4] if not aligned else "fused", k)
        for i in range(3):
            n = 64 * rng.randrange(12, 21) + (0 if aligned else rng.randrange(0, 64))
            specs.append(job(_offset(rng, n, 0 if aligned else 1 + (k + i) % 15), n, (CHAIN if i else INIT) | (FIN if i == 2 else 0),
                             sha, crc))
            dsts.append(lay.abut(n) if i else lay.place(n, 0 if aligned else rng.randrange(0, 16)))
    if case == "every-fifth-null":
        dsts = [None if j % 5 == 2 else d for j, d in enumerate(dsts)]
    states_in, crc_in = _seeded_states(env, rng, 64)
    G = Gather(env, specs, states_in, crc_in, dsts, lay.size)
    G.run()
    due, estatus, img = G.check(case)
    assert due.all() and (estatus == OK).all()
    if case == "every-fifth-null":
        assert sum(d is None for d in dsts) == 38


# ---- 3. block boundaries inside a gathered chain
def test_block_boundaries_inside_a_gathered_chain(env):
    """65 chains of the members {37, 27, 256, 1, 319, 0, 320, 773} in rotated orders, half from INIT and half from
    an in-state with nx = 37 (the head path stores bytes), each gathered contiguously at a seeded alignment: the
    gathered bytes are the concatenation, and hashlib / zlib over the DESTINATION read back give the last
    member's sum."""
    host = env["host"]
    rng = random.Random(1300)
    members = [37, 27, 256, 1, 319, 0, 320, 773]
    lay, specs, dsts, states_in, crc_in, pres, kinds, starts = Layout(), [], [], [], [], [], [], []
    for k in range(65):
        kind = ["fused", "sha", "crc"][k % 3]
        sha, crc = _kinds(kind, k)
        pre = bytes(host[300 * k:300 * k + 64 + 37]) if k % 2 else b""
        pres.append(pre)
        kinds.append(kind)
        states_in.append(state_after(env, pre))
        crc_in.append(zlib.crc32(pre))
        order = members[k % 8:] + members[:k % 8]
        for i, n in enumerate(order):
            specs.append(job(_offset(rng, n), n, (CHAIN if i else (0 if k % 2 else INIT)) | FIN, sha, crc))
            dsts.append(lay.abut(n) if i else lay.place(n, rng.randrange(0, 16)))
        starts.append(dsts[-8])
    G = Gather(env, specs, states_in, crc_in, dsts, lay.size)
    G.run()
    due, estatus, img = G.check("boundaries")
    assert due.all() and (estatus == OK).all()
    _, _, sums, _ = G.A.results()
    total = sum(members)
    for k in range(65):
        want = b"".join(bytes(host[s["off"]:s["off"] + s["n"]]) for s in specs[8 * k:8 * k + 8])
        got = bytes(img[starts[k]:starts[k] + total])
        assert got == want, k
        sha = hashlib.sha1(pres[k] + got).digest() if kinds[k] != "crc" else bytes(20)
        crc = zlib.crc32(got, zlib.crc32(pres[k])).to_bytes(4, "big") if kinds[k] != "sha" else bytes(4)
        assert bytes(sums[8 * k + 7]) == sha + crc, (k, "the last member's sum from the destination")


# ---- 4. ragged extent counts
def test_ragged_extent_counts(env):
    """129 chains of 1-9 members of 0-700 bytes, gathered, with NULL destinations sprinkled in (a NULL member
    leaves its room in the gathered object untouched)."""
    rng = random.Random(1400)
    specs, states_in, crc_in = _ragged(env, rng, 129)
    lay, dsts = Layout(), []
    for j, s in enumerate(specs):
        dsts.append(lay.abut(s["n"]) if s["flags"] & CHAIN else lay.place(s["n"], rng.randrange(0, 16)))
    dsts = [None if rng.randrange(7) == 0 else d for d in dsts]
    assert 20 < sum(d is None for d in dsts) < len(dsts) // 3
    G = Gather(env, specs, states_in, crc_in, dsts, lay.size)
    G.run()
    due, estatus, _ = G.check("ragged")
    assert (estatus == OK).all() and due.all()


# ---- 5. invalid and panicking members
def test_invalid_members_are_not_copied(env):
    """The wide walk's wave of invalidity rules, every member with a destination of its own: EFES_ERR_ARG members
    and the members behind them keep the sentinel, the valid members before them are copied, a job that names
    neither state (valid as a head, hashing nothing) is not copied, the neighbouring chains are exact."""
    specs, bad = _invalid_wave()
    specs += [job(7000, 200, INIT | FIN, None, None), job(9000, 150, INIT | FIN, 63, 63)]  # no state; the next chain
    specs[-1]["sha"] = specs[-1]["crc"] = 64
    states_in, crc_in = _seeded_states(env, random.Random(500), 65)
    lay = Layout()
    dsts = [lay.place(s["n"], (5 * j) % 16) for j, s in enumerate(specs)]
    G = Gather(env, specs, states_in, crc_in, dsts, lay.size)
    G.run()
    due, estatus, img = G.check("invalid")
    assert [j for j in range(len(specs)) if estatus[j] == ARG] == bad
    assert not due[bad].any() and not due[4 * 30] and not due[len(specs) - 2] and due[len(specs) - 1]
    assert np.delete(due, bad + [4 * 30, len(specs) - 2]).all()
    for j in bad + [len(specs) - 2]:
        assert (img[dsts[j] - GUARD:dsts[j] + specs[j]["n"] + GUARD] == SENTINEL).all(), j
    assert due[4 * 5] and due[4 * 5 + 1] and due[4 * 35], "the valid members before an invalid one are copied"


def test_panicking_writes_are_not_copied_and_panicking_sums_are(env):
    """The wide walk's panic wave: nx = 65 at a head (every member EFES_ERR_STATE from its Write: nothing copied,
    for it and the members behind it), nx = -1 (whole blocks: the Sum raises EFES_ERR_STATE with the state
    written, so the member IS copied), EFES_JOB_SUM_ONLY heads (nothing copied), zero-length members."""
    specs, states_in, crc_in, at = _state_wave(env)
    lay = Layout()
    dsts = [lay.place(s["n"], (3 * j) % 16) for j, s in enumerate(specs)]
    G = Gather(env, specs, states_in, crc_in, dsts, lay.size)
    G.run()
    due, estatus, img = G.check("panic states")
    assert estatus[at[3]:at[4]].tolist() == [STATE] * 3 and not due[at[3]:at[4]].any()
    assert estatus[at[7]:at[8]].tolist() == [STATE, OK, STATE] and due[at[7]:at[8]].all()
    assert not due[at[11]] and not due[at[12]]
    assert np.delete(due, [at[3], at[3] + 1, at[3] + 2, at[11], at[12]]).all()
    j = at[7]
    assert bytes(img[dsts[j]:dsts[j] + 128]) == bytes(env["host"][specs[j]["off"]:specs[j]["off"] + 128])


# ---- 6. records
def test_records_on_every_member_and_null_ckpt(env):
    """ckpt_device on every member: the records are efes_hash_chain_wide's (and the oracle's); ckpt_device NULL
    on the same array: the recordless call, the record area untouched."""
    rng = random.Random(1600)
    specs, states_in, crc_in = _ragged(env, rng, 129)
    lay = Layout()
    dsts = [lay.abut(s["n"]) if s["flags"] & CHAIN else lay.place(s["n"], rng.randrange(0, 16)) for s in specs]
    G = Gather(env, specs, states_in, crc_in, dsts, lay.size, ckpt=True)
    G.run()
    G.check("records")
    rec_due, _ = G.A.check_records("records")
    assert rec_due.all()
    N = Gather(env, specs, states_in, crc_in, dsts, lay.size, ckpt=True)
    N.run(with_ckpt=False)
    N.check("NULL ckpt")
    assert (N.A.records() == 0xA5).all()
    same_bytes(G.A, N.A, "with and without records")
    assert G.dst.cpu().numpy().tobytes() == N.dst.cpu().numpy().tobytes()


# ---- 7. more than one wave per SIMD
def test_more_than_one_wave_per_simd(env):
    """66 000 chains of one or two members of 0-130 bytes (about 99 000 jobs: two waves per SIMD on 256 CUs),
    gathered back to back without a byte between the objects: the whole destination against a host-side gather,
    everything else byte for byte efes_hash_chain_wide (the oracle per job would take too long; the wide walk's
    own test ties it to the oracle at this shape)."""
    lib, torch, host = env["lib"], env["torch"], env["host"]
    chains = 66000
    rng = np.random.default_rng(chains)
    members = rng.integers(1, 3, size=chains)
    n = int(members.sum())
    owner = np.repeat(np.arange(chains), members)
    head = np.concatenate(([True], owner[1:] != owner[:-1]))
    lens = rng.integers(0, 131, size=n)
    offs = rng.integers(0, BUF_BYTES - 130, size=n)
    kind = owner % 3
    flags = np.where(head, INIT, CHAIN) | np.where(rng.integers(0, 2, size=n) == 1, FIN, 0)
    specs = [job(int(offs[j]), int(lens[j]), int(flags[j]), int(owner[j]) if kind[j] != 2 else None,
                 int(owner[j]) if kind[j] != 1 else None) for j in range(n)]
    at = GUARD + 3 + np.concatenate(([0], np.cumsum(lens)))  # back to back from an odd address
    size = int(at[-1]) + GUARD
    fresh = np.zeros(chains, dtype=lib.SHA1_STATE_DTYPE)
    G = Gather(env, specs, fresh, np.zeros(chains, np.uint32), [int(a) for a in at[:-1]], size)
    G.run()
    same_bytes(G.A, G.B, chains)
    _, _, _, status = G.A.results()
    assert (status == OK).all()
    want = np.full(size, SENTINEL, dtype=np.uint8)
    idx = np.concatenate([np.arange(o, o + m) for o, m in zip(offs, lens)])
    want[GUARD + 3:GUARD + 3 + idx.size] = host[idx]
    img = G.dst.cpu().numpy()
    bad = np.nonzero(img != want)[0]
    assert bad.size == 0, (bad[:8].tolist(), img[bad[:8]].tolist(), want[bad[:8]].tolist())


# ---- 8. stream order
def test_destination_is_visible_in_stream_order(env):
    """On a side stream: the copy call, then one unflagged INIT | FINALIZE job per object over the GATHERED object
    through efes_hash_chain, with no synchronisation between them: its sums are the chains' last-member sums."""
    torch = env["torch"]
    rng = random.Random(1800)
    lay, specs, dsts, starts, sizes = Layout(), [], [], [], []
    for k in range(70):
        lens = [rng.randrange(0, 2000) for _ in range(1 + k % 4)]
        for i, n in enumerate(lens):
            specs.append(job(_offset(rng, n), n, (CHAIN if i else INIT) | FIN, k, k))
            dsts.append(lay.abut(n) if i else lay.place(n, rng.randrange(0, 16)))
        starts.append(dsts[-len(lens)])
        sizes.append(sum(lens))
    states_in, crc_in = _seeded_states(env, rng, 70)
    G = Gather(env, specs, states_in, crc_in, dsts, lay.size)
    # the second array reads the destination buffer: Chains addresses env["buf"], so its data pointers are re-aimed
    again = [job(0, sizes[k], INIT | FIN, k, k) for k in range(70)]
    fresh = [state_after(env, b"")] * 70
    H = Chains(env, again, fresh, [0] * 70)
    H.rec["data"] = np.array([G.dst.data_ptr() + starts[k] for k in range(70)], dtype=np.uint64)
    H.jobs = torch.from_numpy(H.rec.view(np.uint8).copy()).to("cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device="cuda:0")
    G.submit(stream=stream.cuda_stream)
    H.run(stream=stream.cuda_stream)
    stream.synchronize()
    run_wide(G.B)
    G.check("stream order")
    _, _, sums, _ = G.A.results()
    _, _, hsums, hstatus = H.results()
    assert (hstatus == OK).all()
    last = np.cumsum([1 + k % 4 for k in range(70)]) - 1
    assert hsums.tobytes() == sums[last].tobytes()


# ---- 9. arguments on a live context
def test_arguments(env):
    torch, lib, ctx = env["torch"], env["lib"], env["ctx"]
    L = lib.lib()
    specs = [job(0, 100, INIT | FIN, 0, 0), job(100, 1000, CHAIN | FIN, 0, 0)]
    lay = Layout()
    dsts = [lay.place(100, 3), lay.abut(1000)]
    G = Gather(env, specs, [state_after(env, b"")], [0], dsts, lay.size, ckpt=True)
    C = G.A
    j, d, p, s, nb = C.jobs.data_ptr(), G.ptrs.data_ptr(), C.ptrs.data_ptr(), C.scratch.data_ptr(), C.scratch_bytes
    assert s % 16 == 0
    big = torch.empty(nb + 16, dtype=torch.uint8, device="cuda:0")
    f = L.efes_hash_chain_wide_copy
    for ck in (None, p):
        assert f(ctx.handle, None, None, None, 0, None, 0, None) == lib.EFES_OK
        assert f(ctx.handle, j, d, ck, 0, s, nb, None) == lib.EFES_OK
        assert f(ctx.handle, None, d, ck, 2, s, nb, None) == lib.EFES_ERR_ARG
        assert f(ctx.handle, j, None, ck, 2, s, nb, None) == lib.EFES_ERR_ARG  # NULL dst_device: efes_hash_chain_wide
        assert f(ctx.handle, j, d, ck, 2, None, nb, None) == lib.EFES_ERR_ARG
        assert f(ctx.handle, j, d, ck, 2, big.data_ptr() + 8, nb, None) == lib.EFES_ERR_ARG
        assert f(ctx.handle, j, d, ck, 2, s, nb - 1, None) == lib.EFES_ERR_ARG
        assert f(ctx.handle, j, d, ck, lib.EFES_HASH_CHAIN_MAX_JOBS + 1, s, 1 << 40, None) == lib.EFES_ERR_ARG
    torch.cuda.synchronize()
    assert (C.status.cpu().numpy() == -99).all() and (C.records() == 0xA5).all(), "a refused call launched"
    assert (G.dst.cpu().numpy() == SENTINEL).all(), "a refused call copied"
    G.run()
    G.check("after the refused calls")
    C.check_records("after the refused calls")


# ---- 10. DeviceObjects
@pytest.mark.parametrize("variant", ["fused", "checkpoints", "sha1-only"])
def test_device_objects_wide_copy(env, variant, monkeypatch):
    """70 objects of 0-9 extents with walk="wide" and copy_to=: sha1_hex(), crcs, states_host() (and records)
    against the same set through efes_hash_chain without a copy, against hashlib and zlib, and the gathered bytes
    at copy_offsets with the sentinel everywhere else."""
    batch, lib, ctx, torch, host = env["batch"], env["lib"], env["ctx"], env["torch"], env["host"]
    rng = random.Random(2000)
    objects = [[(rng.randrange(0, BUF_BYTES - 3000), rng.choice([0, rng.randrange(0, 3000)])) for _ in range(k % 10)]
               for k in range(70)]
    kw = dict(sha1=True, running=True, ctx=ctx, checkpoints=variant == "checkpoints", crc32=variant != "sha1-only")
    offsets, room = batch.default_copy_offsets(objects)
    dst = torch.full((room + 2 * batch.COPY_ALIGN,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    calls = []
    orig = type(ctx).hash_chain_wide_copy
    monkeypatch.setattr(type(ctx), "hash_chain_wide_copy", lambda self, *a: calls.append(a[3]) or orig(self, *a))
    O = batch.DeviceObjects(env["buf"].data_ptr(), objects, walk="wide", copy_to=dst.data_ptr() + batch.COPY_ALIGN, **kw)
    P = batch.DeviceObjects(env["buf"].data_ptr(), objects, **kw)
    assert O.copy_offsets.tolist() == offsets.tolist() and O.copy_bytes == room
    O.run()
    P.run()
    assert len(calls) == 1 and (calls[0] is not None) == (variant == "checkpoints")
    assert (O.status_host() == OK).all()
    assert O.states_host().tobytes() == P.states_host().tobytes()
    assert O.sha1_hex() == P.sha1_hex() and O.running_sha1() == P.running_sha1()
    if variant != "sha1-only":
        assert O.crc_sum().tobytes() == P.crc_sum().tobytes()
        assert O.running_crcs().tobytes() == P.running_crcs().tobytes()
    if variant == "checkpoints":
        assert O.checkpoints_host().tobytes() == P.checkpoints_host().tobytes()
    img = dst.cpu().numpy()
    want = np.full(img.size, SENTINEL, dtype=np.uint8)
    sha = O.sha1_hex()
    for k, obj in enumerate(objects):
        whole = b"".join(bytes(host[o:o + n]) for o, n in obj)
        a = batch.COPY_ALIGN + int(O.copy_offsets[k])
        want[a:a + len(whole)] = np.frombuffer(whole, dtype=np.uint8)
        if obj:
            assert sha[k] == hashlib.sha1(whole).hexdigest(), k
            if variant != "sha1-only":
                assert int(O.crc_sum()[k]) == zlib.crc32(whole), k
        else:
            assert sha[k] is None
    assert (img == want).all(), np.nonzero(img != want)[0][:8]
