"""GPU parity of the wide chain walk (efes_hash_chain_wide): one chain per lane, the wavefront walking the
members in rounds.  The yardstick is the chain calls': every case replays each chain as successive write()
calls on the oracle's sha1digest and zlib.crc32 (status, the 104-byte states with their stale bytes, crc,
every FINALIZE member's sum, untouched sentinels), and is compared byte for byte with efes_hash_chain on a
second copy of the inputs; records are compared byte for byte with efes_hash_chain_checkpoints(EFES_MODE_DEEP),
canaries included.  The shapes are the smallest at which the walk takes each of its paths: one wave plus a
lane, two waves plus a lane, the uniform and the ragged bulk phase, aligned and not, lanes that end in
different rounds, a later draw with one live lane, two and three waves per SIMD.  Bit-exact."""
import ctypes
import hashlib
import random
import zlib

import numpy as np
import pytest

from test_gpu_hash_chain import (ARG, BUF_BYTES, CHAIN, FIN, INIT, OK, STATE, SUM_ONLY, Chains, _kinds, _seeded_states,
                                 expectation, job, state_after)
from test_gpu_hash_chain_ckpt import REC, CkptChains, _mixed_array, host_text
from test_gpu_hash_chain_group import same_bytes

pytestmark = pytest.mark.gpu


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


def run_wide(C, ckpt=None, stream="current", scratch=None, first=0, count=None):
    """Chains.run through efes_hash_chain_wide; ckpt: a device pointer array, None for NULL."""
    s = C.env["torch"].cuda.current_stream().cuda_stream if stream == "current" else stream
    scratch = C.scratch if scratch is None else scratch
    count = C.n - first if count is None else count
    C.env["ctx"].hash_chain_wide(C.jobs.data_ptr() + 56 * first, count, ckpt, scratch.data_ptr(), scratch.numel(), s)


def both(env, specs, states_in, crc_in, what):
    """The wide walk on one copy, efes_hash_chain on another: the oracle's expectation, then the same bytes."""
    A, B = Chains(env, specs, states_in, crc_in), Chains(env, specs, states_in, crc_in)
    run_wide(A)
    B.run()
    exp = A.check(what)
    same_bytes(A, B, what)
    return A, exp


def _offset(rng, n, mis=None):
    mis = rng.randrange(0, 16) if mis is None else mis
    return 16 * rng.randrange(0, (BUF_BYTES - n - 16) // 16) + mis


def _kind_of(kind, k):
    return ["fused", "sha", "crc"][k % 3] if kind == "mixed" else kind


# ---- 1. unflagged arrays
@pytest.mark.parametrize("count", [65, 129])
@pytest.mark.parametrize("kind", ["fused", "sha", "crc", "mixed"])
def test_unflagged_array_equals_deep(env, kind, count):
    """65 and 129 unflagged jobs (a full wave plus a lane; two plus one) of 0 ... 5 * 64 + 63 and seeded lengths
    up to 24 blocks at offsets 1-15 mod 16, INIT or resumed with nx in {1, 55, 63, 64}, with and without
    FINALIZE; fused, SHA-1-only, CRC-only and the three mixed in one wave: efes_hash_chain's bytes and
    efes_hash_submit_mode(EFES_MODE_DEEP)'s."""
    rng = random.Random(100 * count + len(kind))
    host = env["host"]
    lengths = [0, 1, 63, 64, 65, 127, 128, 129, 5 * 64 + 63]
    specs, states_in, crc_in = [], [], []
    for k in range(count):
        n = lengths[k] if k < len(lengths) else rng.choice([rng.randrange(0, 24 * 64 + 1), rng.choice(lengths)])
        sha, crc = _kinds(_kind_of(kind, k), k)
        flags = rng.choice([0, FIN])
        nx = [None, 1, 55, 63, 64][(k + k // 5) % 5]
        if nx is None:
            flags |= INIT
            states_in.append(state_after(env, b""))
        else:
            pre = 64 * rng.randrange(0, 3) + (63 if nx == 64 else nx)
            states_in.append(state_after(env, bytes(host[k * 256:k * 256 + pre]), nx))
        crc_in.append(rng.getrandbits(32))
        specs.append(job(_offset(rng, n, 1 + k % 15), n, flags, sha, crc))
    A, _ = both(env, specs, states_in, crc_in, (kind, count))
    D = Chains(env, specs, states_in, crc_in)
    D.run_deep()
    same_bytes(A, D, (kind, count, "EFES_MODE_DEEP"))


# ---- 2. the uniform phase of the bulk loop
@pytest.mark.parametrize("aligned", [True, False])
def test_uniform_phase(env, aligned):
    """64 chains x 3 members of 12-20 blocks, every lane of the wave live, so the shortest member leaves the
    bulk loop a uniform phase (b + 5 < nmin) in every round.  Aligned: 16-byte aligned extents of whole blocks
    from INIT, so every round's first bulk byte is aligned in every lane; misaligned: offsets at 1-15 mod 16 and
    lengths with tails."""
    rng = random.Random(200 + aligned)
    specs = []
    for k in range(64):
        sha, crc = _kinds(["fused", "fused", "sha", "crc"][k % 4] if not aligned else "fused", k)
        for i in range(3):
            n = 64 * rng.randrange(12, 21) + (0 if aligned else rng.randrange(0, 64))
            specs.append(job(_offset(rng, n, 0 if aligned else 1 + (k + i) % 15), n, (CHAIN if i else INIT) | (FIN if i == 2 else 0),
                             sha, crc))
    states_in, crc_in = _seeded_states(env, rng, 64)
    both(env, specs, states_in, crc_in, ("uniform", aligned))


# ---- 3. block boundaries inside a chain
def test_block_boundaries_inside_a_chain(env):
    """65 chains of the members {37, 27, 256, 1, 319, 0, 320, 773} in rotated orders, the running digest after
    every member, from INIT or from an in-state with nx = 37; hashlib and zlib over each prefix are the second
    check."""
    host = env["host"]
    rng = random.Random(300)
    members = [37, 27, 256, 1, 319, 0, 320, 773]
    specs, states_in, crc_in, pres, kinds = [], [], [], [], []
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
    _, (_, _, esums, estatus) = both(env, specs, states_in, crc_in, "boundaries")
    assert (estatus == OK).all()
    for k in range(65):
        h, crc = hashlib.sha1(pres[k]), zlib.crc32(pres[k])
        for j in range(8 * k, 8 * k + 8):
            data = bytes(host[specs[j]["off"]:specs[j]["off"] + specs[j]["n"]])
            h.update(data)
            crc = zlib.crc32(data, crc)
            want = (h.digest() if kinds[k] != "crc" else bytes(20)) + (crc.to_bytes(4, "big") if kinds[k] != "sha" else bytes(4))
            assert bytes(esums[j]) == want, (k, j)


# ---- 4. ragged extent counts in one wave
def _ragged(env, rng, chains):
    """`chains` chains of 1-9 members of 0-700 bytes, zero-length members among them, kinds and starts mixed."""
    specs = []
    for k in range(chains):
        sha, crc = _kinds(["fused", "sha", "crc"][k % 3], k)
        for i in range(1 + (k * 7 + k // 9) % 9):
            n = rng.choice([0, rng.randrange(0, 130), rng.randrange(0, 701)])
            specs.append(job(_offset(rng, n), n, (CHAIN if i else rng.choice([0, INIT])) | rng.choice([0, FIN]), sha, crc))
    states_in, crc_in = _seeded_states(env, rng, chains)
    return specs, states_in, crc_in


def test_ragged_extent_counts(env):
    """64 chains of 1-9 members: the lanes of one wave finish in different rounds.  129 chains: the wave that
    draws the third ticket has one live lane.  Then both again back to back on one stream and one scratch: every
    call re-zeroes the ticket."""
    torch = env["torch"]
    rng = random.Random(400)
    a, b = _ragged(env, rng, 64), _ragged(env, rng, 129)
    assert {1 + (k * 7 + k // 9) % 9 for k in range(64)} == set(range(1, 10))
    assert sum(1 for s in a[0] if s["n"] == 0) >= 10
    both(env, *a, "64 chains")
    both(env, *b, "129 chains")
    sets = [Chains(env, *b), Chains(env, *a), Chains(env, *b)]
    shared = torch.empty(max(c.scratch_bytes for c in sets), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    for c in sets:
        run_wide(c, stream=stream.cuda_stream, scratch=shared)
    for c, what in zip(sets, ("first", "second", "third")):
        c.check(("shared scratch", what))


# ---- 5. every invalidity rule, each in another lane of one wave
def _invalid_wave():
    """64 chains of 4 members over states 0..63 (state 64: the other state of the pointer rules); the rules sit
    in chains 0, 5, 10, ... with valid chains between them.  Returns (specs, jobs that must get EFES_ERR_ARG)."""
    specs = []
    for k in range(64):
        specs += [job(3000 * k + 197 * i, 50 + 13 * i + k, (CHAIN if i else INIT) | FIN, k, k) for i in range(4)]
    bad = []
    specs[0]["flags"] |= CHAIN  # a flagged job 0: lane 0 of the wave
    bad += [0, 1, 2, 3]
    specs[4 * 5 + 2]["sha"] = 64
    bad += [4 * 5 + 2, 4 * 5 + 3]
    specs[4 * 10 + 2]["crc"] = 64
    bad += [4 * 10 + 2, 4 * 10 + 3]
    specs[4 * 15 + 1]["sha"] = specs[4 * 15 + 1]["crc"] = None
    bad += [4 * 15 + 1, 4 * 15 + 2, 4 * 15 + 3]
    specs[4 * 20 + 3]["flags"] |= INIT
    bad += [4 * 20 + 3]
    specs[4 * 25 + 2]["flags"] |= SUM_ONLY
    specs[4 * 25 + 2]["n"] = 0
    bad += [4 * 25 + 2, 4 * 25 + 3]
    specs[4 * 30]["flags"], specs[4 * 30]["n"] = FIN | SUM_ONLY, 0  # its followers are invalid
    bad += [4 * 30 + 1, 4 * 30 + 2, 4 * 30 + 3]
    specs[4 * 35 + 1]["crc"] = 64  # invalid by itself; the members behind it name the chain's states again
    bad += [4 * 35 + 1, 4 * 35 + 2, 4 * 35 + 3]
    return specs, sorted(bad)


def test_invalid_members(env):
    """EFES_ERR_ARG for each rule's member and the members behind it, their sums untouched, the members before
    them in effect and the state as after the last valid one (the oracle's expectation), the other state never
    written, the neighbouring chains exact."""
    specs, bad = _invalid_wave()
    states_in, crc_in = _seeded_states(env, random.Random(500), 65)
    A, (_, _, esums, estatus) = both(env, specs, states_in, crc_in, "invalid")
    assert [j for j in range(len(specs)) if estatus[j] == ARG] == bad
    assert (np.delete(estatus, bad) == OK).all()
    assert (esums[bad] == 0xA5).all()
    states, crcs, _, _ = A.results()
    assert states[64].tobytes() == A.states_in[64].tobytes() and crcs[64] == A.crc_in[64], "the other state was written"
    assert states[30].tobytes() == A.states_in[30].tobytes() and crcs[30] == A.crc_in[30], "a SUM_ONLY head stored its state"


# ---- 6. EFES_ERR_STATE
def _state_wave(env):
    """20 chains: nx = 65 at the head of chain 3 (every member EFES_ERR_STATE, nothing written), nx = -1 at the
    head of chain 7 (whole blocks only: Sum panics with the state written), SUM_ONLY heads in chains 11 and 12,
    zero-length FINALIZE members in chains 15 and 16, valid chains between them.  Returns the specs, the
    in-states and each chain's first job."""
    host = env["host"]
    rng = random.Random(600)
    states_in, crc_in = _seeded_states(env, rng, 20)
    states_in[3] = state_after(env, bytes(host[:64 + 20]))
    states_in[3]["nx"] = 65
    states_in[7] = state_after(env, bytes(host[:64 + 20]))
    states_in[7]["nx"] = -1
    specs, at = [], []
    for k in range(20):
        at.append(len(specs))
        if k == 3:
            specs += [job(300 + 70 * i, 70, (CHAIN if i else 0) | FIN, k, k) for i in range(3)]
        elif k == 7:
            specs += [job(900 + 128 * i, [128, 0, 64][i], (CHAIN if i else 0) | (FIN if i != 1 else 0), k, k) for i in range(3)]
        elif k == 11:
            specs += [job(5000, 77, FIN | SUM_ONLY, k, k)]  # the Sum of the in-state plus 77 bytes, on a copy
        elif k == 12:
            specs += [job(0, 0, FIN | SUM_ONLY, k, k)]
        else:
            lens = {15: [91, 0, 92], 16: [0, 93, 0]}.get(k, [90 + k, 91 + k, 92 + k])
            specs += [job(_offset(rng, n), n, (CHAIN if i else INIT) | FIN, k, k) for i, n in enumerate(lens)]
    return specs, states_in, crc_in, at


def test_go_panic_states(env):
    specs, states_in, crc_in, at = _state_wave(env)
    A, (_, _, esums, estatus) = both(env, specs, states_in, crc_in, "panic states")
    assert estatus[at[3]:at[4]].tolist() == [STATE] * 3 and (esums[at[3]:at[4]] == 0xA5).all()
    assert estatus[at[7]:at[8]].tolist() == [STATE, OK, STATE]
    assert (np.delete(estatus, [at[3], at[3] + 1, at[3] + 2, at[7], at[7] + 2]) == OK).all()
    states, crcs, _, _ = A.results()
    for k in (3, 11, 12):  # a panicking Write and SUM_ONLY heads: the states are never written
        assert states[k].tobytes() == A.states_in[k].tobytes() and crcs[k] == A.crc_in[k], k
    assert int(states[7]["nx"]) == -1 and int(states[7]["len"]) == int(A.states_in[7]["len"]) + 192


# ---- 7. checkpoints
def _ckpt_pair(env, specs, states_in, crc_in, null=None, what=""):
    """The wide walk with records on one copy, efes_hash_chain_checkpoints(EFES_MODE_DEEP) on another: the
    oracle's records, then the same bytes in everything written and in the whole record area."""
    W, D = CkptChains(env, specs, states_in, crc_in, null=null), CkptChains(env, specs, states_in, crc_in, null=null)
    run_wide(W, ckpt=W.ptrs.data_ptr())
    D.run_ckpt(env["lib"].MODE_DEEP)
    exp = W.check(what)
    due, recs = W.check_records(what)
    same_bytes(W, D, what)
    assert W.records().tobytes() == D.records().tobytes(), (what, "records")
    return W, exp, due


def test_checkpoints_on_every_member(env):
    specs, states_in, crc_in = _ragged(env, random.Random(700), 129)
    _, (_, _, _, estatus), due = _ckpt_pair(env, specs, states_in, crc_in, what="every member")
    assert (estatus == OK).all() and due.all()


def test_checkpoints_null_entries_invalid_and_panicking_members(env):
    """The checkpoint tests' mixed array (about 300 jobs, every invalidity rule, a Write that panics, a Sum that
    panics, SUM_ONLY, in-state _pad words that are not zero) with ckpt[j] == NULL for every third member, then
    this file's invalid and panic waves: records not due and the guard bytes keep every 0xA5."""
    specs, states_in, crc_in, rules = _mixed_array(env)
    null = np.arange(len(specs)) % 3 == 1
    _, (_, _, _, estatus), due = _ckpt_pair(env, specs, states_in, crc_in, null=null, what="mixed")
    assert estatus[rules["write-panic"]] == STATE and not due[rules["write-panic"]]
    assert estatus[rules["sum-panic"]] == STATE and due[rules["sum-panic"]]
    assert estatus[rules["other-sha1"]] == ARG and not due[rules["other-sha1"]]
    assert (due & ~null).sum() > 100 and (due & null).sum() > 50 and (~due & ~null).sum() >= 8
    specs, bad = _invalid_wave()
    states_in, crc_in = _seeded_states(env, random.Random(500), 65)
    _, _, due = _ckpt_pair(env, specs, states_in, crc_in, what="invalid wave")
    assert not due[bad].any() and not due[4 * 30] and np.delete(due, bad + [4 * 30]).all()
    specs, states_in, crc_in, at = _state_wave(env)
    _, _, due = _ckpt_pair(env, specs, states_in, crc_in, what="panic wave")
    assert not due[at[3]:at[4]].any() and due[at[7]:at[8]].all() and not due[at[11]] and not due[at[12]]


def test_null_ckpt_is_the_recordless_call(env):
    specs, states_in, crc_in = _ragged(env, random.Random(710), 70)
    W, N = CkptChains(env, specs, states_in, crc_in), CkptChains(env, specs, states_in, crc_in)
    run_wide(W, ckpt=W.ptrs.data_ptr())
    run_wide(N, ckpt=None)
    N.check("NULL ckpt")
    same_bytes(W, N, "NULL ckpt")
    assert (N.records() == 0xA5).all()
    W.check_records("with ckpt")


def test_resume_from_a_mid_chain_record(env):
    """70 chains of 4 members cut after the second: the rest, without INIT, from copies of that member's record
    through efes_hash_chain_wide equals the uncut chains."""
    lib = env["lib"]
    rng = random.Random(720)
    specs = []
    for k in range(70):
        sha, crc = _kinds(["fused", "sha", "crc"][k % 3], k)
        for i in range(4):
            n = rng.randrange(0, 400)
            specs.append(job(_offset(rng, n), n, (CHAIN if i else INIT) | FIN, sha, crc))
    states_in, crc_in = _seeded_states(env, rng, 70)
    U = Chains(env, specs, states_in, crc_in)
    run_wide(U)
    U.check("uncut")
    first = [s for k in range(70) for s in specs[4 * k:4 * k + 2]]
    rest = []
    for k in range(70):
        a, b = dict(specs[4 * k + 2]), dict(specs[4 * k + 3])
        a["flags"] &= ~(CHAIN | INIT)
        rest += [a, b]
    F = CkptChains(env, first, states_in, crc_in, stride=REC)
    run_wide(F, ckpt=F.ptrs.data_ptr())
    F.check_records("first half")
    cut = F.records()[:F.n * REC].view(lib.CHECKPOINT_DTYPE)[1::2]
    R = Chains(env, rest, cut["sha1"].copy(), cut["crc"].copy())
    run_wide(R)
    R.check("second half")
    su, cu, sumu, _ = U.results()
    sr, cr, sumr, _ = R.results()
    for k in range(70):
        kind = ["fused", "sha", "crc"][k % 3]
        assert bytes(sumr[2 * k]) == bytes(sumu[4 * k + 2]) and bytes(sumr[2 * k + 1]) == bytes(sumu[4 * k + 3]), k
        if kind != "crc":
            for f in ("h", "x", "nx", "len"):
                assert sr[k][f].tolist() == su[k][f].tolist(), (k, f)
        if kind != "sha":
            assert cr[k] == cu[k], k


# ---- 8. more than one wave per SIMD
@pytest.mark.parametrize("chains", [66000, 140000])
def test_more_than_one_wave_per_simd(env, chains):
    """66 000 and 140 000 chains of 1-2 members of 0-130 bytes: about 99 000 and 210 000 jobs, so on 256 CUs
    (1024 SIMDs of 64 lanes) the launcher asks for 2 and 3 waves per SIMD.  With the kernel's 147 VGPRs and
    117 808 B of LDS at three waves the runtime admits the three, so it picks wps = 2 and wps = 3 (workgroups of
    512 and 768 lanes).  Byte for byte efes_hash_chain_mode(EFES_MODE_GROUP4) only -- the oracle per job would
    take too long -- with the oracle on 64 seeded chains of the array."""
    lib = env["lib"]
    rng = np.random.default_rng(chains)
    members = rng.integers(1, 3, size=chains)
    n = int(members.sum())
    owner = np.repeat(np.arange(chains), members)
    head = np.concatenate(([True], owner[1:] != owner[:-1]))
    lens = rng.integers(0, 131, size=n)
    offs = rng.integers(0, BUF_BYTES - 130, size=n)
    kind = owner % 3  # fused, SHA-1-only, CRC-only
    flags = np.where(head, INIT, CHAIN) | np.where(rng.integers(0, 2, size=n) == 1, FIN, 0)
    specs = [job(int(offs[j]), int(lens[j]), int(flags[j]), int(owner[j]) if kind[j] != 2 else None,
                 int(owner[j]) if kind[j] != 1 else None) for j in range(n)]
    fresh = np.zeros(chains, dtype=lib.SHA1_STATE_DTYPE)
    crc_in = np.zeros(chains, np.uint32)
    A, B = Chains(env, specs, fresh, crc_in), Chains(env, specs, fresh, crc_in)
    run_wide(A)
    env["ctx"].hash_chain_mode(B.jobs.data_ptr(), B.n, B.scratch.data_ptr(), B.scratch.numel(),
                               env["torch"].cuda.current_stream().cuda_stream, lib.MODE_GROUP[4])
    same_bytes(A, B, chains)
    states, crcs, sums, status = A.results()
    assert (status == OK).all()
    first = np.nonzero(head)[0]
    for c in random.Random(chains).sample(range(chains), 64):  # the oracle on 64 seeded chains
        lo, hi = int(first[c]), int(first[c]) + int(members[c])
        sub = [dict(s, sha=None if s["sha"] is None else 0, crc=None if s["crc"] is None else 0) for s in specs[lo:hi]]
        es, ec, esum, est = expectation(env, sub, fresh[:1], crc_in[:1])
        assert (status[lo:hi] == est).all() and (sums[lo:hi] == esum).all(), c
        for f in ("h", "x", "nx", "len"):
            assert states[c][f].tolist() == es[0][f].tolist(), (c, f)
        assert crcs[c] == ec[0], c


def test_waves_the_chain_count_cannot_fill_leave(env):
    """20 000 chains x 4 members of 0-40 bytes: 80 000 jobs make the launcher ask for two waves per SIMD on 256
    CUs, and 313 waves of chains fill less than one, so in every workgroup the second wave of each SIMD leaves
    behind the barrier and the first ones do all the work.  Byte for byte efes_hash_chain_mode(EFES_MODE_GROUP4),
    the oracle on 64 seeded chains, records on every member byte for byte efes_hash_chain_checkpoints'."""
    lib = env["lib"]
    chains = 20000
    rng = np.random.default_rng(chains)
    n = 4 * chains
    owner = np.repeat(np.arange(chains), 4)
    lens = rng.integers(0, 41, size=n)
    offs = rng.integers(0, BUF_BYTES - 40, size=n)
    kind = owner % 3
    flags = np.where(np.arange(n) % 4 == 0, INIT, CHAIN) | np.where(rng.integers(0, 2, size=n) == 1, FIN, 0)
    specs = [job(int(offs[j]), int(lens[j]), int(flags[j]), int(owner[j]) if kind[j] != 2 else None,
                 int(owner[j]) if kind[j] != 1 else None) for j in range(n)]
    fresh = np.zeros(chains, dtype=lib.SHA1_STATE_DTYPE)
    crc_in = np.zeros(chains, np.uint32)
    A, B = CkptChains(env, specs, fresh, crc_in, stride=REC), CkptChains(env, specs, fresh, crc_in, stride=REC)
    run_wide(A, ckpt=A.ptrs.data_ptr())
    B.run_ckpt(lib.MODE_GROUP[4])
    same_bytes(A, B, "leaving waves")
    assert A.records().tobytes() == B.records().tobytes()
    states, crcs, sums, status = A.results()
    assert (status == OK).all()
    for c in random.Random(chains).sample(range(chains), 64):
        sub = [dict(s, sha=None if s["sha"] is None else 0, crc=None if s["crc"] is None else 0) for s in specs[4 * c:4 * c + 4]]
        es, ec, esum, est = expectation(env, sub, fresh[:1], crc_in[:1])
        assert (status[4 * c:4 * c + 4] == est).all() and (sums[4 * c:4 * c + 4] == esum).all(), c
        for f in ("h", "x", "nx", "len"):
            assert states[c][f].tolist() == es[0][f].tolist(), (c, f)
        assert crcs[c] == ec[0], c


# ---- 9. arguments
def test_arguments(env):
    torch, lib, ctx = env["torch"], env["lib"], env["ctx"]
    L = lib.lib()
    specs = [job(0, 100, INIT | FIN, 0, 0), job(100, 1000, CHAIN | FIN, 0, 0)]
    C = CkptChains(env, specs, [state_after(env, b"")], [0])
    j, p, s, nb = C.jobs.data_ptr(), C.ptrs.data_ptr(), C.scratch.data_ptr(), C.scratch_bytes
    assert s % 16 == 0
    big = torch.empty(nb + 16, dtype=torch.uint8, device="cuda:0")
    for ck in (None, p):
        assert L.efes_hash_chain_wide(ctx.handle, None, 0, None, None, 0, None) == lib.EFES_OK
        assert L.efes_hash_chain_wide(ctx.handle, j, 0, ck, s, nb, None) == lib.EFES_OK
        assert L.efes_hash_chain_wide(ctx.handle, None, 2, ck, s, nb, None) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_wide(ctx.handle, j, 2, ck, None, nb, None) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_wide(ctx.handle, j, 2, ck, big.data_ptr() + 8, nb, None) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_wide(ctx.handle, j, 2, ck, s, nb - 1, None) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_wide(ctx.handle, j, lib.EFES_HASH_CHAIN_MAX_JOBS + 1, ck, s, 1 << 40, None) == lib.EFES_ERR_ARG
    torch.cuda.synchronize()
    assert (C.status.cpu().numpy() == -99).all() and (C.records() == 0xA5).all(), "a refused call launched"
    W = Chains(env, specs, [state_after(env, b"")], [0])
    W.run()
    run_wide(C, ckpt=p)
    C.check("after the refused calls")
    C.check_records("after the refused calls")
    same_bytes(C, W, "after the refused calls")


# ---- 10. DeviceObjects
@pytest.mark.parametrize("checkpoints", [False, True])
@pytest.mark.parametrize("walk", ["wide", "auto_wide"])
def test_device_objects_walk(env, walk, checkpoints, monkeypatch):
    """70 objects of 0-9 extents with walk="wide" / "auto_wide" against the same set with walk=None: sums,
    states, CRCs, statuses and records; the records' texts round-trip through the host codecs."""
    batch, lib, ctx = env["batch"], env["lib"], env["ctx"]
    rng = random.Random(1000)
    objects = [[(rng.randrange(0, BUF_BYTES - 3000), rng.choice([0, rng.randrange(0, 3000)])) for _ in range(k % 10)]
               for k in range(70)]
    calls = []
    orig = type(ctx).hash_chain_wide
    monkeypatch.setattr(type(ctx), "hash_chain_wide", lambda self, *a: calls.append(a[2]) or orig(self, *a))
    O = batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, running=True, checkpoints=checkpoints, walk=walk, ctx=ctx)
    P = batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, running=True, checkpoints=checkpoints, ctx=ctx)
    O.run()
    P.run()
    nwith = sum(1 for o in objects if o)
    if walk == "wide" or env["hashing"].hash_chain_auto_mode_wide(nwith, ctx) == lib.MODE_WIDE:
        assert len(calls) == 1 and (calls[0] is not None) == checkpoints
    else:
        assert calls == [] and O.walk == env["hashing"].hash_chain_auto_mode(nwith, ctx)
    assert (O.status_host() == OK).all()
    assert O.status_host().tobytes() == P.status_host().tobytes()
    assert O.states_host().tobytes() == P.states_host().tobytes()
    assert O.crc_sum().tobytes() == P.crc_sum().tobytes()
    assert O.sha1_hex() == P.sha1_hex() and O.running_sha1() == P.running_sha1()
    assert O.running_crcs().tobytes() == P.running_crcs().tobytes()
    if checkpoints:
        ck = O.checkpoints_host()
        assert ck.tobytes() == P.checkpoints_host().tobytes()
        texts = O.checkpoint_texts()
        assert len(texts) == O.n
        for j in range(O.n):
            t = host_text(lib, ck[j])
            assert texts[j] == (t[:200], t[200:]), j
        st = lib.Sha1State()
        assert lib.lib().efes_sha1_state_unmarshal_text(ctypes.byref(st), texts[-1][0], 200) == lib.EFES_OK
        assert bytes(st)[:84] == ck[-1]["sha1"].tobytes()[:84] and st.nx == int(ck[-1]["sha1"]["nx"]) and st.len == int(ck[-1]["sha1"]["len"])
