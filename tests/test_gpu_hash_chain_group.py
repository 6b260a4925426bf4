"""GPU parity of the grouped chain walk (efes_hash_chain_mode with EFES_MODE_GROUPn): 64/G chains per
wavefront, G lanes each, for more chains than SIMDs.  Every case is checked twice: against the oracle's
successive Writes (status, the full 104-byte state with its stale bytes, crc, every FINALIZE member's sum, the
sentinels of invalid members), and byte for byte against efes_hash_chain on a second copy of the same array.
Bit-exact.  A wave's first draw takes 64/G consecutive chains, so the first 64/G chains of an array share a
wave and meet in joint rounds whenever their members have G whole blocks left."""
import hashlib
import random
import zlib

import numpy as np
import pytest

from test_gpu_hash_chain import (ARG, BUF_BYTES, CHAIN, FIN, INIT, OK, STATE, SUM_ONLY, Chains, _kinds, _seeded_states,
                                 expectation, job, state_after)

pytestmark = pytest.mark.gpu

GS = [4, 8, 16, 32]
WHAT = ("state", "crc", "sum", "status")


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
                host=buf.cpu().numpy(), cus=torch.cuda.get_device_properties(0).multi_processor_count)


def run_mode(C, mode, stream="current", scratch=None, first=0, count=None):
    """Chains.run through efes_hash_chain_mode."""
    s = C.env["torch"].cuda.current_stream().cuda_stream if stream == "current" else stream
    scratch = C.scratch if scratch is None else scratch
    count = C.n - first if count is None else count
    C.env["ctx"].hash_chain_mode(C.jobs.data_ptr() + 56 * first, count, scratch.data_ptr(), scratch.numel(), s, mode)


def same_bytes(A, B, what):
    for a, b, f in zip(A.results(), B.results(), WHAT):
        assert a.tobytes() == b.tobytes(), (what, f)


def both(env, specs, states_in, crc_in, G, what):
    """The grouped walk on one copy, efes_hash_chain on another: the oracle's expectation, then the same bytes."""
    A, B = Chains(env, specs, states_in, crc_in), Chains(env, specs, states_in, crc_in)
    run_mode(A, env["lib"].MODE_GROUP[G])
    B.run()
    exp = A.check((what, G))
    same_bytes(A, B, (what, G))
    return A, exp


def _offset(rng, n, mis=None):
    """A data offset with n bytes behind it, at `mis` mod 16 (None: seeded)."""
    mis = rng.randrange(0, 16) if mis is None else mis
    return 16 * rng.randrange(0, (BUF_BYTES - n - 16) // 16) + mis


# ---- 1. unflagged arrays
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("kind", ["fused", "sha", "crc"])
def test_unflagged_array_equals_deep(env, kind, G):
    """Arrays of 3 * (64/G) + 1 unflagged jobs at unaligned offsets, lengths around the block and the G-block
    super-step, INIT or resumed from mid-block states, with and without FINALIZE: what EFES_MODE_DEEP writes."""
    rng = random.Random(1000 * G + len(kind))
    B = 64 * G
    lengths = [0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 63] + [rng.randrange(0, 6 * B + 1) for _ in range(4)]
    per = 3 * (64 // G) + 1
    while len(lengths) % per:
        lengths.append(lengths[len(lengths) % 13])
    host = env["host"]
    for a in range(len(lengths) // per):
        specs, states_in, crc_in = [], [], []
        for k, n in enumerate(lengths[a * per:(a + 1) * per]):
            sha, crc = _kinds(kind, k)
            flags = rng.choice([0, FIN])
            nx = [None, 1, 55, 63, 64][(k + a) % 5]
            if nx is None:
                flags |= INIT
                states_in.append(state_after(env, b""))
            else:
                pre = 64 * rng.randrange(0, 3) + (63 if nx == 64 else nx)
                states_in.append(state_after(env, bytes(host[k * 256:k * 256 + pre]), nx))
            crc_in.append(rng.getrandbits(32))
            specs.append(job(_offset(rng, n, 1 + k % 15), n, flags, sha, crc))
        A, _ = both(env, specs, states_in, crc_in, G, (kind, a))
        D = Chains(env, specs, states_in, crc_in)
        D.run_deep()
        same_bytes(A, D, (kind, G, a, "EFES_MODE_DEEP"))


# ---- 2. block boundaries inside a chain
@pytest.mark.parametrize("G", GS)
def test_block_boundaries_inside_a_chain(env, G):
    """64/G + 1 chains of the same eight members in rotated orders, FINALIZE on every member, heads with INIT
    and heads resuming a state with nx = 37: nx carries across members and across joint rounds, and the
    joiners differ from round to round.  hashlib / zlib over each prefix are the second check."""
    rng = random.Random(200 + G)
    host = env["host"]
    B = 64 * G
    members = [37, 27, B, 1, B + 63, 0, 5 * 64, 3 * B + 5]
    pre = bytes(host[100:100 + 64 + 37])
    specs, states_in, crc_in = [], [], []
    for k in range(64 // G + 1):
        init = k % 2 == 0
        states_in.append(state_after(env, b"" if init else pre, None if init else 37))
        crc_in.append(0 if init else zlib.crc32(pre))
        for i in range(len(members)):
            n = members[(i + k) % len(members)]
            specs.append(job(_offset(rng, n, [0, 1, 3, 15][(i + k) % 4]), n, (CHAIN if i else (INIT if init else 0)) | FIN, k, k))
    _, (_, _, esums, estatus) = both(env, specs, states_in, crc_in, G, "boundaries")
    assert (estatus == OK).all()
    for k in range(64 // G + 1):
        h, crc = (hashlib.sha1(), 0) if k % 2 == 0 else (hashlib.sha1(pre), zlib.crc32(pre))
        for j in range(8 * k, 8 * k + 8):
            data = bytes(host[specs[j]["off"]:specs[j]["off"] + specs[j]["n"]])
            h.update(data)
            crc = zlib.crc32(data, crc)
            assert bytes(esums[j]) == h.digest() + crc.to_bytes(4, "big"), (G, k, j)


# ---- 3. slot counts
@pytest.mark.parametrize("G", GS)
def test_slot_counts(env, G):
    """1, 2, 64/G - 1, 64/G and 64/G + 1 chains of one to three members of up to four super-steps: dead
    slots, a lone joiner on the one-job path, a full wave, and one chain more than a wave holds."""
    rng = random.Random(300 + G)
    k = 64 // G
    for chains in sorted({1, 2, k - 1, k, k + 1} - {0}):
        specs = []
        for c in range(chains):
            for i in range(1 + (c + chains) % 3):
                n = rng.choice([64 * G, 2 * 64 * G + 17, rng.randrange(64 * G, 4 * 64 * G), rng.randrange(0, 64 * G)])
                specs.append(job(_offset(rng, n), n, (CHAIN if i else rng.choice([0, INIT])) | rng.choice([0, FIN]), c, c))
        states_in, crc_in = _seeded_states(env, rng, chains)
        both(env, specs, states_in, crc_in, G, ("slots", chains))


# ---- 4. more chains than resident slots
@pytest.mark.parametrize("G", GS)
def test_more_chains_than_resident_slots(env, G):
    """multi_processor_count * 4 * (64/G) + 37 chains of 2 members of 1 to 2 * 64 G + 200 bytes: every slot of
    every resident wave holds a chain and some draw again.  All digests against hashlib and zlib, len and nx
    of every state, and the whole result against efes_hash_chain."""
    host, lib = env["host"], env["lib"]
    rng = np.random.default_rng(4000 + G)
    nobj = env["cus"] * 4 * (64 // G) + 37
    top = 2 * 64 * G + 200
    lens = rng.integers(1, top + 1, size=2 * nobj)
    offs = rng.integers(0, BUF_BYTES - top, size=2 * nobj)
    objects = [[(int(offs[2 * i]), int(lens[2 * i])), (int(offs[2 * i + 1]), int(lens[2 * i + 1]))] for i in range(nobj)]
    O = env["batch"].DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, ctx=env["ctx"], walk=lib.MODE_GROUP[G])
    W = env["batch"].DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, ctx=env["ctx"])
    O.run()
    W.run()
    assert (O.status_host() == OK).all()
    sha, crc = O.sha1_hex(), O.crc_sum()
    for i, ((a, n), (b, m)) in enumerate(objects):
        data = bytes(host[a:a + n]) + bytes(host[b:b + m])
        assert sha[i] == hashlib.sha1(data).hexdigest(), i
        assert int(crc[i]) == zlib.crc32(data), i
    st = O.states_host()
    assert (st["len"] == lens.reshape(nobj, 2).sum(axis=1)).all() and (st["nx"] == st["len"] % 64).all()
    for f in ("states", "crcs", "sums", "status"):
        assert getattr(O, f).cpu().numpy().tobytes() == getattr(W, f).cpu().numpy().tobytes(), f


# ---- 5. mixed kinds
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("mix", ["mixed", "sha", "crc"])
def test_mixed_kinds(env, mix, G):
    """Fused, SHA-1-only and CRC-only chains side by side in one wave (any_sha and any_crc from different
    slots), an all-SHA-1 array at 16-byte-aligned data only, and an all-CRC array; the mixed and the CRC
    arrays hold aligned and unaligned data in the same wave."""
    rng = random.Random(500 + G + len(mix))
    k = 64 // G
    specs = []
    for c in range(2 * k):
        kind = ["fused", "sha", "crc"][c % 3] if mix == "mixed" else mix
        sha, crc = _kinds(kind, c)
        for i in range(3):
            n = rng.randrange(2 * 64 * G, 5 * 64 * G) if i != 1 else 64 * rng.randrange(G, 3 * G)
            mis = 0 if mix == "sha" or (c + i) % 2 == 0 else rng.randrange(1, 16)
            specs.append(job(_offset(rng, n, mis), n, (CHAIN if i else INIT) | (FIN if i != 1 else 0), sha, crc))
    states_in, crc_in = _seeded_states(env, rng, 2 * k)
    both(env, specs, states_in, crc_in, G, mix)


# ---- 6. invalid members
def _invalid_case_long(rule, G):
    """test_gpu_hash_chain._invalid_case with members of two to three super-steps: four chains over states
    0..3 (+4: another state), the rule's member at job 4, in the middle of chain 1 (jobs 2-7)."""
    def chain(k, members, head=INIT):
        return [job(200000 * k + 20011 * i, 2 * 64 * G + 50 + 13 * i, (CHAIN if i else head) | FIN, k, k) for i in range(members)]
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


@pytest.mark.parametrize("G", [4, 32])
@pytest.mark.parametrize("rule", ["flagged-job-0", "other-sha1", "other-crc32", "both-null", "with-init", "with-sum-only",
                                  "after-sum-only-head", "after-invalid-member"])
def test_invalid_members(env, rule, G):
    """One case per rule of efes_hash.h, the invalid member between members long enough to join rounds:
    EFES_ERR_ARG for it and every member behind it, their sums and the neighbours' statuses intact, the states
    as after the valid prefix, the chains in the other slots correct."""
    specs, bad = _invalid_case_long(rule, G)
    rng = random.Random(len(rule))
    states_in, crc_in = _seeded_states(env, rng, 5)
    A, (_, _, esums, estatus) = both(env, specs, states_in, crc_in, G, rule)
    assert [j for j in range(len(specs)) if estatus[j] == ARG] == bad, (rule, estatus)
    assert (esums[bad] == 0xA5).all()
    assert all(estatus[j] == OK for j in range(len(specs)) if j not in bad)
    states, crcs, _, _ = A.results()
    assert states[4].tobytes() == A.states_in[4].tobytes() and crcs[4] == A.crc_in[4], "the other state was written"


# ---- 7. Go's panic states
@pytest.mark.parametrize("G", [4, 32])
def test_go_panic_states(env, G):
    """nx = 65 at a Write: EFES_ERR_STATE on every member, the state untouched.  nx = -1: Sum panics, the
    state is written.  Beside them an EFES_JOB_SUM_ONLY head, a chain of zero-length members only, a head with
    FINALIZE and length 0, and an ordinary chain that joins rounds with the nx = -1 chain."""
    host = env["host"]
    B = 64 * G
    s65, sneg = state_after(env, bytes(host[:64 + 20])), state_after(env, bytes(host[:64 + 20]))
    s65["nx"], sneg["nx"] = 65, -1
    specs = [job(300 + 70 * i, 70, (CHAIN if i else 0) | FIN, 0, 0) for i in range(3)]
    specs += [job(900 + 3 * B * i, [2 * B, 0, B + 64][i], (CHAIN if i else 0) | (FIN if i != 1 else 0), 1, 1) for i in range(3)]
    specs += [job(5000, 0, FIN | SUM_ONLY, 2, 2)]
    specs += [job(6000 + i, 0, (CHAIN if i else 0) | (FIN if i == 2 else 0), 3, 3) for i in range(3)]
    specs += [job(7000, 0, INIT | FIN, 4, 4)]
    specs += [job(50001 + 4 * B * i, 3 * B + 9, (CHAIN if i else INIT) | FIN, 5, 5) for i in range(2)]
    mid = state_after(env, bytes(host[64:64 + 100]))
    A, (_, _, esums, estatus) = both(env, specs, [s65, sneg, mid, mid, mid, mid], [0x12345678, 0x9ABCDEF0, 3, 4, 5, 6], G, "panic")
    assert estatus.tolist() == [STATE, STATE, STATE, STATE, OK, STATE] + [OK] * 7
    assert (esums[:3] == 0xA5).all()
    states, crcs, _, _ = A.results()
    assert states[0].tobytes() == s65.tobytes() and crcs[0] == 0x12345678
    assert states[2].tobytes() == mid.tobytes() and crcs[2] == 3, "a Sum-only job wrote its state"


# ---- 8. one long chain of short members beside ordinary chains
def test_long_chain_of_short_members_beside_joiners(env):
    """G = 4: a chain of 2049 members of 7 bytes as chain 5 of 17, the other 16 with members of many
    super-steps: one slot's refill loop runs long while the wave's other slots hold joinable members."""
    G = 4
    rng = random.Random(2049)
    specs, c = [], 0

    def ordinary(c):
        return [job(_offset(rng, 9000), rng.randrange(3000, 9000), (CHAIN if i else INIT) | FIN, c, c) for i in range(3)]
    for c in range(5):
        specs += ordinary(c)
    specs += [job(3 + 11 * i, 7, (CHAIN if i else 0) | (FIN if i % 97 == 0 or i == 2048 else 0), 5, 5) for i in range(2049)]
    for c in range(6, 64 // G + 1):
        specs += ordinary(c)
    states_in, crc_in = _seeded_states(env, rng, 64 // G + 1)
    both(env, specs, states_in, crc_in, G, "2049 members")


# ---- 9. arguments
def test_arguments(env):
    torch, lib, ctx = env["torch"], env["lib"], env["ctx"]
    L = lib.lib()
    specs = [job(0, 100, INIT | FIN, 0, 0), job(100, 1000, CHAIN | FIN, 0, 0)]
    C = Chains(env, specs, [state_after(env, b"")], [0])
    j, s, nb = C.jobs.data_ptr(), C.scratch.data_ptr(), C.scratch_bytes
    assert s % 16 == 0
    for mode in (lib.MODE_AUTO, lib.MODE_WIDE, lib.MODE_FED4, lib.MODE_FED4E, -1, 99):
        assert L.efes_hash_chain_mode(ctx.handle, j, 2, s, nb, None, mode) == lib.EFES_ERR_ARG, mode
        assert L.efes_hash_chain_mode(ctx.handle, None, 0, None, 0, None, mode) == lib.EFES_ERR_ARG, mode
    big = torch.empty(nb + 16, dtype=torch.uint8, device="cuda:0")
    for mode in [lib.MODE_DEEP] + [lib.MODE_GROUP[G] for G in GS]:
        assert L.efes_hash_chain_mode(ctx.handle, None, 0, None, 0, None, mode) == lib.EFES_OK
        assert L.efes_hash_chain_mode(ctx.handle, j, 0, s, nb, None, mode) == lib.EFES_OK
        assert L.efes_hash_chain_mode(ctx.handle, None, 2, s, nb, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_mode(ctx.handle, j, 2, None, nb, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_mode(ctx.handle, j, 2, big.data_ptr() + 8, nb, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_mode(ctx.handle, j, 2, s, nb - 1, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_mode(ctx.handle, j, lib.EFES_HASH_CHAIN_MAX_JOBS + 1, s, 1 << 40, None, mode) == lib.EFES_ERR_ARG
    torch.cuda.synchronize()
    assert (C.status.cpu().numpy() == -99).all(), "a refused call launched"
    D, W = Chains(env, specs, [state_after(env, b"")], [0]), Chains(env, specs, [state_after(env, b"")], [0])
    run_mode(D, lib.MODE_DEEP)
    W.run()
    D.check("EFES_MODE_DEEP")
    same_bytes(D, W, "EFES_MODE_DEEP")
    run_mode(C, lib.MODE_GROUP[8])
    C.check("after the refused calls")


# ---- 10. streams and scratch
def test_streams_and_scratch(env):
    """A grouped call and a wave-walk call back to back on one stream over one scratch buffer (both orders);
    two grouped calls on two streams with a scratch each; a call over a sub-range whose first job carries
    EFES_JOB_CHAIN: it is job 0 of the call, so it and its followers are invalid."""
    torch, lib = env["torch"], env["lib"]
    rng = random.Random(1010)

    def make(chains, G):
        specs = []
        for k in range(chains):
            for i in range(rng.randrange(1, 4)):
                n = rng.randrange(0, 3 * 64 * G)
                specs.append(job(_offset(rng, n), n, (CHAIN if i else INIT) | FIN, k, k))
        states_in, crc_in = _seeded_states(env, rng, chains)
        return Chains(env, specs, states_in, crc_in)

    sa, sb = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    sets = [make(40, 16), make(300, 16), make(7, 4), make(90, 4)]
    shared = torch.empty(max(c.scratch_bytes for c in sets), dtype=torch.uint8, device="cuda:0")
    run_mode(sets[0], lib.MODE_GROUP[16], sa.cuda_stream, scratch=shared)
    sets[1].run(sa.cuda_stream, scratch=shared)
    run_mode(sets[2], lib.MODE_GROUP[4], sa.cuda_stream, scratch=shared)
    sets[3].run(sa.cuda_stream, scratch=shared)
    for c, what in zip(sets, ("group16", "wave", "group4", "wave again")):
        c.check(what)
    A, B = make(300, 8), make(200, 32)
    run_mode(A, lib.MODE_GROUP[8], sa.cuda_stream)
    run_mode(B, lib.MODE_GROUP[32], sb.cuda_stream)
    A.check("stream a")
    B.check("stream b")

    # a sub-range [first, first + count) that starts inside a chain
    G = 8
    specs = []
    for k in range(6):
        for i in range(4):
            n = 64 * G + 100 * i + k
            specs.append(job(_offset(rng, n), n, (CHAIN if i else INIT) | FIN, k, k))
    states_in, crc_in = _seeded_states(env, rng, 6)
    first, count = 6, 13  # job 6 is member 2 of chain 1; the range ends inside chain 4
    assert specs[first]["flags"] & CHAIN
    S, W = Chains(env, specs, states_in, crc_in), Chains(env, specs, states_in, crc_in)
    run_mode(S, lib.MODE_GROUP[G], first=first, count=count)
    W.run(first=first, count=count)
    same_bytes(S, W, "sub-range")
    estates, ecrcs, esums, estatus = expectation(env, specs[first:first + count], S.states_in, S.crc_in)
    states, crcs, sums, status = S.results()
    assert estatus[:2].tolist() == [ARG, ARG] and (estatus[2:] == OK).all()
    assert status[first:first + count].tolist() == estatus.tolist()
    assert (status[:first] == -99).all() and (status[first + count:] == -99).all()
    assert sums[first:first + count].tobytes() == esums.tobytes()
    assert (sums[:first] == 0xA5).all() and (sums[first + count:] == 0xA5).all()
    for f in ("h", "x", "nx", "len"):
        assert states[f].tolist() == estates[f].tolist(), f
    assert crcs.tolist() == ecrcs.tolist()


# ---- 11. DeviceObjects
@pytest.mark.parametrize("walk", ["auto", "group8"])
def test_device_objects_walk(env, walk, monkeypatch):
    """DeviceObjects(sha1=True, walk=...): objects of 0, 1 and 9 extents with running digests equal hashlib and
    zlib at every extent; walk goes through efes_hash_chain_mode; walk with sha1=False is refused."""
    host, batch, lib, ctx = env["host"], env["batch"], env["lib"], env["ctx"]
    ext9 = [(20000 + 1031 * i, [0, 1, 63, 64, 65, 700, 4096, 5, 129][i]) for i in range(9)]
    objects = [[], [(100, 777)], ext9]
    calls = []
    orig = type(ctx).hash_chain_mode
    monkeypatch.setattr(type(ctx), "hash_chain_mode", lambda self, *a: calls.append(a[-1]) or orig(self, *a))
    O = batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, running=True, ctx=ctx,
                            walk="auto" if walk == "auto" else lib.MODE_GROUP[8])
    O.run()
    assert calls == [env["hashing"].hash_chain_auto_mode(2, ctx) if walk == "auto" else lib.MODE_GROUP[8]]
    assert (O.status_host() == OK).all() and O.status_host().size == 10
    cat = [b"".join(bytes(host[a:a + n]) for a, n in o) for o in objects]
    assert O.sha1_hex() == [None] + [hashlib.sha1(c).hexdigest() for c in cat[1:]]
    assert O.crc_sum().tolist() == [0] + [zlib.crc32(c) for c in cat[1:]]
    run_sha, run_crc, h, crc = [], [], hashlib.sha1(), 0
    for a, n in ext9:
        h.update(bytes(host[a:a + n]))
        crc = zlib.crc32(bytes(host[a:a + n]), crc)
        run_sha.append(h.hexdigest())
        run_crc.append(crc)
    assert O.running_sha1() == [hashlib.sha1(cat[1]).hexdigest()] + run_sha
    assert O.running_crcs().tolist() == [zlib.crc32(cat[1])] + run_crc
    st = O.states_host()
    assert st[0].tobytes() == batch.fresh_states(1)[0].tobytes()  # no extents: no job, the in-state kept
    with pytest.raises(ValueError):
        batch.DeviceObjects(env["buf"].data_ptr(), objects, ctx=ctx, walk="auto")
    with pytest.raises(ValueError):
        batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=False, ctx=ctx, walk=lib.MODE_GROUP[8])
