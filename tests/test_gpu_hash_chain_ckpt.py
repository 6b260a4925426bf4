"""GPU parity of the checkpoint calls (efes_hash_chain_checkpoints, efes_checkpoints_marshal_text): the
resumable state after every member of a chain, what `.info` holds after each PATCH.  The yardstick is the
chain calls': each chain replayed as successive write() calls on the oracle's sha1digest and zlib.crc32, the
record of member j being the full state after that Write (h, all 64 bytes of x, nx, len; the _pad fields 0)
and the CRC, all zero for the hash a chain does not keep.  Records and the bytes around them are pre-filled
with 0xA5: a record that is not due, and every guard byte, keeps them.  Everything else the call writes is
compared byte for byte with efes_hash_chain_mode on a copy of the inputs.  Bit-exact."""
import ctypes
import hashlib
import json
import os
import random
import zlib

import numpy as np
import pytest

from test_gpu_hash_chain import (ARG, BOUNDARY_LENGTHS, BUF_BYTES, CHAIN, FIN, INIT, OK, STATE, SUM_ONLY, Chains, _kinds,
                                 _oracle_of, _row_of, _seeded_chains, _seeded_states, job, state_after)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ["deep", 4, 8, 16, 32]
WHAT = ("state", "crc", "sum", "status")
REC, TEXT = 112, 208


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


def mode_of(env, m):
    return env["lib"].MODE_DEEP if m == "deep" else env["lib"].MODE_GROUP[m]


def ckpt_expectation(env, specs, states_in, crc_in):
    """(due, records): for every job whether a checkpoint is due, and the CHECKPOINT_DTYPE record it must hold
    -- the oracle's state and zlib's CRC after that member's Write, by the validity rules of efes_hash.h."""
    lib, host = env["lib"], env["host"]
    states = np.array(states_in, dtype=lib.SHA1_STATE_DTYPE)
    crcs = [int(c) for c in crc_in]
    due = np.zeros(len(specs), dtype=bool)
    recs = np.zeros(len(specs), dtype=lib.CHECKPOINT_DTYPE)
    bad, prev = False, None
    for j, s in enumerate(specs):
        if s["flags"] & CHAIN:
            bad = (bad or j == 0 or s["sha"] != prev["sha"] or s["crc"] != prev["crc"] or
                   (s["sha"] is None and s["crc"] is None) or bool(s["flags"] & (INIT | SUM_ONLY)) or
                   bool(prev["flags"] & SUM_ONLY))
        else:
            bad = False
        prev = s
        if bad or s["flags"] & SUM_ONLY:
            continue
        data = bytes(host[s["off"]:s["off"] + s["n"]])
        if s["sha"] is not None:
            d = env["oracle"].Sha1() if s["flags"] & INIT else _oracle_of(env, states[s["sha"]])
            if d.write(data):  # Go panics in the Write: nothing of this member is written
                continue
            states[s["sha"]] = _row_of(env, d)
            recs[j]["sha1"] = states[s["sha"]]
            recs[j]["sha1"]["_pad"] = 0
        if s["crc"] is not None:
            crcs[s["crc"]] = zlib.crc32(data, 0 if s["flags"] & INIT else crcs[s["crc"]])
            recs[j]["crc"] = crcs[s["crc"]]
        due[j] = True
    return due, recs


class CkptChains(Chains):
    """Chains with one record slot per job at `stride` bytes (>= 112; the bytes between records are guards),
    everything pre-filled with 0xA5, and the device pointer array (0 where `null` is set)."""

    def __init__(self, env, specs, states_in, crc_in, stride=128, null=None):
        super().__init__(env, specs, states_in, crc_in)
        torch = env["torch"]
        self.stride = stride
        self.null = np.zeros(self.n, dtype=bool) if null is None else np.asarray(null, dtype=bool)
        self.recs = torch.full((max(self.n, 1) * stride + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        assert self.recs.data_ptr() % 8 == 0 and stride % 8 == 0
        at = np.uint64(self.recs.data_ptr()) + np.arange(self.n, dtype=np.uint64) * np.uint64(stride)
        at[self.null] = 0
        self.ptrs = torch.from_numpy(at.view(np.uint8).copy()).to("cuda:0") if self.n else torch.zeros(8, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def run_ckpt(self, mode, stream="current", scratch=None, first=0, count=None):
        s = self.env["torch"].cuda.current_stream().cuda_stream if stream == "current" else stream
        scratch = self.scratch if scratch is None else scratch
        count = self.n - first if count is None else count
        self.env["ctx"].hash_chain_checkpoints(self.jobs.data_ptr() + 56 * first, count, self.ptrs.data_ptr() + 8 * first,
                                               scratch.data_ptr(), scratch.numel(), s, mode)

    def records(self):
        self.env["torch"].cuda.synchronize()
        return self.recs.cpu().numpy()

    def check_records(self, what=""):
        """Records due hold the expectation; everything else under the record area keeps its 0xA5."""
        due, exp = ckpt_expectation(self.env, self.specs, self.states_in, self.crc_in)
        raw = self.records()
        rows = raw[:self.n * self.stride].reshape(self.n, self.stride)
        want = np.full_like(rows, 0xA5)
        written = due & ~self.null
        want[written, :REC] = exp[written].view(np.uint8).reshape(-1, REC)
        bad = np.nonzero((rows != want).any(axis=1))[0]
        assert bad.size == 0, (what, "record", [(int(j), self.specs[j], bool(written[j]), bytes(rows[j]).hex(), bytes(want[j]).hex())
                                                for j in bad[:3]])
        assert (raw[self.n * self.stride:] == 0xA5).all(), (what, "bytes behind the last record")
        return due, exp


def same_bytes(A, B, what):
    for a, b, f in zip(A.results(), B.results(), WHAT):
        assert a.tobytes() == b.tobytes(), (what, f)


def host_text(lib, rec) -> bytes:
    """The 208 characters of one record by the host codecs (the specification)."""
    raw = np.asarray(rec).tobytes()
    st, cs = lib.Sha1State.from_buffer_copy(raw[:104]), lib.Crc32State.from_buffer_copy(raw[104:108])
    a, b = ctypes.create_string_buffer(200), ctypes.create_string_buffer(8)
    lib.lib().efes_sha1_state_marshal_text(ctypes.byref(st), a)
    lib.lib().efes_crc32_state_marshal_text(ctypes.byref(cs), b)
    return a.raw + b.raw


def device_texts(env, ptr, n, guard=TEXT):
    """n records at ptr through efes_checkpoints_marshal_text: (n, 208) characters; the guard row behind them
    must keep its fill."""
    torch = env["torch"]
    text = torch.full((n * TEXT + guard,), 0x7E, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()  # the fill is on torch's stream, the launch on the context's
    env["ctx"].checkpoints_marshal_text(ptr, n, text.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    t = text.cpu().numpy()
    assert (t[n * TEXT:] == 0x7E).all(), "the text launch wrote behind its n * 208 characters"
    return t[:n * TEXT].reshape(n, TEXT)


def _offset(rng, n, mis=None):
    mis = rng.randrange(0, 16) if mis is None else mis
    return 16 * rng.randrange(0, (BUF_BYTES - n - 16) // 16) + mis


# ---- 1. golden texts
@pytest.mark.parametrize("m", MODES)
def test_golden_texts(env, m):
    """Every case of tests/golden/sha1_states.json as one SHA-1 chain (reset: false from the zero-value state
    without INIT) and every case of crc32_states.json as one CRC chain, all in ONE call, every extent with a
    checkpoint: the device-marshalled text of member k equals texts[k], character for character."""
    torch, lib = env["torch"], env["lib"]
    sha_cases = json.load(open(os.path.join(GOLDEN, "sha1_states.json")))
    crc_cases = json.load(open(os.path.join(GOLDEN, "crc32_states.json")))
    blob, specs, want = bytearray(), [], []
    for k, c in enumerate(sha_cases + crc_cases):
        is_sha = k < len(sha_cases)
        for i, w in enumerate(c["writes"]):
            data = bytes.fromhex(w)
            head = INIT if (not is_sha or c["reset"]) else 0
            specs.append(job(len(blob), len(data), (CHAIN if i else head) | FIN, k if is_sha else None, None if is_sha else k))
            want.append((is_sha, c["texts"][i]))
            blob += data
        blob += bytes(1)  # the next case starts at another offset mod 16
    assert len(want) >= 60
    gold = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).to("cuda:0")
    genv = dict(env, buf=gold, host=gold.cpu().numpy())
    nstates = len(sha_cases) + len(crc_cases)
    C = CkptChains(genv, specs, np.zeros(nstates, dtype=lib.SHA1_STATE_DTYPE), np.zeros(nstates, np.uint32), stride=REC)
    C.run_ckpt(mode_of(env, m))
    C.check(("golden", m))
    due, _ = C.check_records(("golden", m))
    assert due.all()
    texts = device_texts(env, C.recs.data_ptr(), C.n)
    for j, (is_sha, t) in enumerate(want):
        got = bytes(texts[j])
        if is_sha:
            assert got[:200].decode() == t and got[200:] == b"0" * 8, (m, j)
        else:
            assert got[200:].decode() == t and got[:200] == b"0" * 200, (m, j)


# ---- 2. block boundaries
def _boundary_object(kind, flags_head):
    specs, off = [], 4096
    for i, n in enumerate(BOUNDARY_LENGTHS):
        off = (off + 15) // 16 * 16 + [0, 1, 3, 15][i % 4]
        sha, crc = _kinds(kind, 0)
        specs.append(job(off, n, (CHAIN if i else flags_head) | FIN, sha, crc))
        off += n
    return specs


@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("kind,start", [("fused", "init"), ("fused", "nx37"), ("sha", "init"), ("sha", "nx37"), ("crc", "init"),
                                        ("crc", "nx37")])
def test_block_boundaries(env, kind, start, m):
    """The BOUNDARY_LENGTHS object (0 ... 65 539 bytes) at data offsets 0, 1, 3, 15 mod 16: every checkpoint is
    the oracle's state after that Write and zlib's CRC, the hash the chain does not keep all zero; hashlib over
    the prefix is the second check (the record's state finalised on the host).  EFES_MODE_DEEP: also byte for
    byte the states read back after each of k successive efes_hash_submit_mode(EFES_MODE_DEEP) calls."""
    torch, lib, host = env["torch"], env["lib"], env["host"]
    pre = bytes(host[100:100 + 64 + 37]) if start == "nx37" else b""
    specs = _boundary_object(kind, INIT if start == "init" else 0)
    ins = ([state_after(env, pre)], [zlib.crc32(pre)])
    C = CkptChains(env, specs, *ins)
    C.run_ckpt(mode_of(env, m))
    _, _, _, estatus = C.check((kind, start, m))
    assert (estatus == OK).all()
    due, exp = C.check_records((kind, start, m))
    assert due.all()
    h, crc = hashlib.sha1(pre), zlib.crc32(pre)
    for j, s in enumerate(specs):
        data = bytes(host[s["off"]:s["off"] + s["n"]])
        h.update(data)
        crc = zlib.crc32(data, crc)
        if kind != "sha":
            assert int(exp[j]["crc"]) == crc
        else:
            assert int(exp[j]["crc"]) == 0
        if kind != "crc":
            rc, dig = _oracle_of(env, exp[j]["sha1"]).sum()
            assert rc == 0 and dig == h.digest(), (kind, start, j)
        else:
            assert exp[j]["sha1"].tobytes() == bytes(104)
    if m != "deep":
        return
    D = Chains(env, specs, *ins)  # the yardstick itself: one job per call, the states read back after each
    stream = torch.cuda.current_stream().cuda_stream
    snaps = []
    for j in range(D.n):
        env["ctx"].submit(D.jobs.data_ptr() + 56 * j, 1, stream, lib.MODE_DEEP)
        torch.cuda.synchronize()  # the null stream handle is the context's own, non-blocking stream
        snaps.append((D.states.cpu().numpy().copy(), D.crcs.cpu().numpy().copy()))
    rows = C.records()[:C.n * C.stride].reshape(C.n, C.stride)
    for j, (st, cs) in enumerate(snaps):
        st = st.view(lib.SHA1_STATE_DTYPE)[0].copy()
        st["_pad"] = 0
        want = (st.tobytes() if kind != "crc" else bytes(104)) + (cs.view(np.uint32)[:1].tobytes() if kind != "sha" else bytes(4))
        assert bytes(rows[j, :108]) == want, (kind, start, j)


# ---- 3. joint rounds and refills / 5. resume
def _round_chains(env, m, rng):
    """2 * (64/G) + 1 chains of 3 members of 3*G*64 + 17 bytes and one of G*64 - 1: members advance in joint
    rounds, finish on the one-job path, and slots draw new chains.  Kinds and starts (INIT / an in-state with
    nx = 37) alternate.  Returns (specs, states_in, crc_in, prefixes)."""
    host = env["host"]
    G = 32 if m == "deep" else m
    chains = 2 * (64 // G) + 1
    specs, states_in, crc_in, pres = [], [], [], []
    for k in range(chains):
        kind = ["fused", "sha", "crc"][k % 3]
        sha, crc = _kinds(kind, k)
        pre = bytes(host[300 * k:300 * k + 64 + 37]) if k % 2 else b""
        pres.append(pre)
        states_in.append(state_after(env, pre))
        crc_in.append(zlib.crc32(pre))
        for i, n in enumerate([3 * G * 64 + 17] * 3 + [G * 64 - 1]):
            specs.append(job(_offset(rng, n), n, (CHAIN if i else (0 if k % 2 else INIT)) | FIN, sha, crc))
    return specs, states_in, crc_in, pres


@pytest.mark.parametrize("m", MODES)
def test_joint_rounds_and_refills(env, m):
    specs, states_in, crc_in, _ = _round_chains(env, m, random.Random(303))
    A, B = CkptChains(env, specs, states_in, crc_in), Chains(env, specs, states_in, crc_in)
    A.run_ckpt(mode_of(env, m))
    env["ctx"].hash_chain_mode(B.jobs.data_ptr(), B.n, B.scratch.data_ptr(), B.scratch.numel(),
                               env["torch"].cuda.current_stream().cuda_stream, mode_of(env, m))
    _, _, _, estatus = A.check(("rounds", m))
    assert (estatus == OK).all()
    same_bytes(A, B, ("rounds", m))
    due, _ = A.check_records(("rounds", m))
    assert due.all()


@pytest.mark.parametrize("m", MODES)
def test_resume_from_checkpoints(env, m):
    """Every chain of the joint-round case cut after its second member; in a second call the remaining members
    start, without INIT, from copies of that member's checkpoint: final states, CRCs and FINALIZE sums equal the
    uncut run's, and hashlib's and zlib's over the whole object."""
    lib, host = env["lib"], env["host"]
    specs, states_in, crc_in, pres = _round_chains(env, m, random.Random(505))
    U = CkptChains(env, specs, states_in, crc_in)  # uncut
    U.run_ckpt(mode_of(env, m))
    U.check(("uncut", m))
    U.check_records(("uncut", m))
    nch = len(specs) // 4
    first = [s for k in range(nch) for s in specs[4 * k:4 * k + 2]]
    rest = []
    for k in range(nch):
        a, b = dict(specs[4 * k + 2]), dict(specs[4 * k + 3])
        a["flags"] &= ~(CHAIN | INIT)
        rest += [a, b]
    F = CkptChains(env, first, states_in, crc_in, stride=REC)
    F.run_ckpt(mode_of(env, m))
    F.check(("first half", m))
    cut = F.records()[:F.n * REC].view(lib.CHECKPOINT_DTYPE)[1::2]  # each chain's second member
    R = CkptChains(env, rest, cut["sha1"].copy(), cut["crc"].copy())
    R.run_ckpt(mode_of(env, m))
    R.check(("second half", m))
    su, cu, sumu, _ = U.results()
    sr, cr, sumr, _ = R.results()
    for k in range(nch):
        kind = ["fused", "sha", "crc"][k % 3]
        data = pres[k] + b"".join(bytes(host[s["off"]:s["off"] + s["n"]]) for s in specs[4 * k:4 * k + 4])
        assert bytes(sumr[2 * k]) == bytes(sumu[4 * k + 2]) and bytes(sumr[2 * k + 1]) == bytes(sumu[4 * k + 3]), (m, k)
        want = (hashlib.sha1(data).digest() if kind != "crc" else bytes(20)) + (zlib.crc32(data).to_bytes(4, "big") if kind != "sha" else bytes(4))
        assert bytes(sumr[2 * k + 1]) == want, (m, k)
        if kind != "crc":
            for f in ("h", "x", "nx", "len"):
                assert sr[k][f].tolist() == su[k][f].tolist(), (m, k, f)
        if kind != "sha":
            assert cr[k] == cu[k] == zlib.crc32(data), (m, k)


# ---- 4. nothing else changes, nothing extra is written
def _mixed_array(env):
    """About 300 jobs: seeded chains of 1-5 members of 0-300 bytes, then one invalid member of every kind the
    header lists, in-states with nx = 64 and nx > 64, a SUM_ONLY head with followers, a lone SUM_ONLY job,
    zero-length members, in-state _pad words that are not zero."""
    rng = random.Random(404)
    host = env["host"]
    specs, k = _seeded_chains(rng, 300)
    states_in, crc_in = _seeded_states(env, rng, k + 1)  # state k: the "other" state of the pointer rules
    for row in states_in[::2]:
        row["_pad"] = 0xDEADBEEF
    starts = [j for j, s in enumerate(specs) if not s["flags"] & CHAIN]
    lens = [b - a for a, b in zip(starts, starts[1:] + [len(specs)])]
    long3 = [a for a, n in zip(starts, lens) if n >= 3 and a > 0]
    one = [a for a, n in zip(starts, lens) if n == 1 and a > 0]
    assert len(long3) >= 9 and len(one) >= 2

    def fuse(a):  # make the chain at job a a fused one (for the rules that need both pointers); its state
        kk = specs[a]["sha"] if specs[a]["sha"] is not None else specs[a]["crc"]
        j = a
        while j < len(specs) and (j == a or specs[j]["flags"] & CHAIN):
            specs[j]["sha"], specs[j]["crc"] = kk, kk
            j += 1
        return kk
    rules = {"flagged-job-0": 0, "other-sha1": long3[0] + 1, "other-crc32": long3[1] + 1, "both-null": long3[2] + 1,
             "with-init": long3[3] + 1, "with-sum-only": long3[4] + 1, "after-sum-only-head": long3[5] + 1,
             "write-panic": long3[7], "sum-panic": long3[8], "lone-sum-only": one[0]}
    specs[0]["flags"] |= CHAIN
    fuse(long3[0])
    specs[rules["other-sha1"]]["sha"] = k
    fuse(long3[1])
    specs[rules["other-crc32"]]["crc"] = k
    specs[rules["both-null"]]["sha"] = specs[rules["both-null"]]["crc"] = None
    specs[rules["with-init"]]["flags"] |= INIT
    specs[rules["with-sum-only"]]["flags"] |= SUM_ONLY | FIN
    specs[rules["with-sum-only"]]["n"] = 0
    specs[long3[5]]["flags"], specs[long3[5]]["n"] = FIN | SUM_ONLY, 0  # a SUM_ONLY head: its followers are invalid
    specs[long3[6]]["flags"] = FIN  # an in-state with nx = 64: the pending block completes at the first byte
    states_in[fuse(long3[6])] = state_after(env, bytes(host[:64 + 63]), 64)
    specs[long3[7]]["flags"] = FIN  # nx = 65: Go panics at every Write
    states_in[fuse(long3[7])] = state_after(env, bytes(host[:64 + 20]))
    states_in[specs[long3[7]]["sha"]]["nx"] = 65
    states_in[fuse(long3[8])] = state_after(env, bytes(host[:64 + 20]))  # nx = -1: the state is written, Sum panics
    states_in[specs[long3[8]]["sha"]]["nx"] = -1
    specs[long3[8]]["flags"] = 0
    for i, n in enumerate([128, 0, 64]):  # whole blocks only: nx stays -1
        specs[long3[8] + i].update(off=900 + 128 * i, n=n)
        specs[long3[8] + i]["flags"] |= FIN
    specs[one[0]]["flags"], specs[one[0]]["n"] = FIN | SUM_ONLY, 0
    assert sum(1 for s in specs if s["n"] == 0) >= 3
    return specs, states_in, crc_in, rules


@pytest.mark.parametrize("m", MODES)
def test_nothing_else_changes_nothing_extra_written(env, m):
    """States, CRCs, sums and statuses byte-identical to efes_hash_chain_mode(mode) on copies of the same
    inputs; the records due are correct; records not due -- a NULL entry's neighbours, EFES_ERR_ARG, a Write
    that panics, SUM_ONLY -- and the 16 guard bytes between records at a stride of 128 keep every 0xA5."""
    specs, states_in, crc_in, rules = _mixed_array(env)
    null = np.arange(len(specs)) % 3 == 1
    A, B = CkptChains(env, specs, states_in, crc_in, null=null), Chains(env, specs, states_in, crc_in)
    A.run_ckpt(mode_of(env, m))
    env["ctx"].hash_chain_mode(B.jobs.data_ptr(), B.n, B.scratch.data_ptr(), B.scratch.numel(),
                               env["torch"].cuda.current_stream().cuda_stream, mode_of(env, m))
    _, _, _, estatus = A.check(("mixed", m))
    same_bytes(A, B, ("mixed", m))
    due, _ = A.check_records(("mixed", m))
    for rule in ("flagged-job-0", "other-sha1", "other-crc32", "both-null", "with-init", "with-sum-only", "after-sum-only-head"):
        j = rules[rule]
        assert estatus[j] == ARG and not due[j], rule
        if specs[j + 1]["flags"] & CHAIN:  # the members behind an invalid one are invalid too
            assert estatus[j + 1] == ARG and not due[j + 1], rule
    j = rules["write-panic"]
    assert (estatus[j:j + 3] == STATE).all() and not due[j:j + 3].any()
    j = rules["sum-panic"]
    assert (estatus[j:j + 3] == STATE).all() and due[j:j + 3].all(), "Sum panics with the state written: a record is due"
    assert not due[rules["lone-sum-only"]] and not due[rules["after-sum-only-head"] - 1]
    assert (due & ~null).sum() > 100 and (due & null).sum() > 50 and (~due & ~null).sum() >= 8


# ---- 6. more chains than resident slots, shared scratch
@pytest.mark.parametrize("m", ["deep", 4])
def test_more_chains_than_slots_shared_scratch(env, m):
    """3 000 chains of 2 members of 65-200 bytes, two calls back to back on one stream sharing one scratch."""
    torch = env["torch"]
    sets = []
    for seed in (3000, 3001):
        rng = random.Random(seed)
        specs = []
        for k in range(3000):
            sha, crc = _kinds(["fused", "sha", "crc"][k % 3], k)
            for i in range(2):
                n = rng.randrange(65, 201)
                specs.append(job(rng.randrange(0, BUF_BYTES - n), n, (CHAIN if i else INIT) | (FIN if i else 0), sha, crc))
        fresh = np.zeros(3000, dtype=env["lib"].SHA1_STATE_DTYPE)
        sets.append(CkptChains(env, specs, fresh, np.zeros(3000, np.uint32), stride=REC))
    shared = torch.empty(max(c.scratch_bytes for c in sets), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream(device="cuda:0")
    for c in sets:
        c.run_ckpt(mode_of(env, m), stream=stream.cuda_stream, scratch=shared)
    for c, what in zip(sets, ("first", "second")):
        c.check((what, m))
        due, _ = c.check_records((what, m))
        assert due.all()


# ---- 7. DeviceObjects
@pytest.mark.parametrize("walk", [None, "auto"])
def test_device_objects_checkpoints(env, walk, monkeypatch):
    host, batch, lib = env["host"], env["batch"], env["lib"]
    ext9 = [(20000 + 1031 * i, [0, 1, 63, 64, 65, 700, 4096, 5, 129][i]) for i in range(9)]
    objects = [[], [(100, 777)], ext9, [(50000, 64), (60000, 0), (70001, 191)]]
    calls = []
    ctx = env["ctx"]
    orig = type(ctx).hash_chain_checkpoints
    monkeypatch.setattr(type(ctx), "hash_chain_checkpoints", lambda self, *a: calls.append(a[-1]) or orig(self, *a))
    O = batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, checkpoints=True, walk=walk, ctx=ctx)
    O.run()
    assert calls == [lib.MODE_DEEP], "always efes_hash_chain_checkpoints; 3 objects: the wave walk either way"
    assert (O.status_host() == OK).all() and O.status_host().size == 13
    ck, texts = O.checkpoints_host(), O.checkpoint_texts()
    assert ck.dtype == lib.CHECKPOINT_DTYPE and ck.size == 13 and len(texts) == 13
    j = 0
    for o in objects:
        d, crc = env["oracle"].Sha1(), 0
        for a, n in o:
            assert d.write(bytes(host[a:a + n])) == 0
            crc = zlib.crc32(bytes(host[a:a + n]), crc)
            want = np.zeros(1, dtype=lib.CHECKPOINT_DTYPE)[0]
            want["sha1"], want["crc"] = _row_of(env, d), crc
            assert ck[j].tobytes() == want.tobytes(), j
            t = host_text(lib, ck[j])
            assert texts[j] == (t[:200], t[200:]) and isinstance(texts[j][0], bytes), j
            j += 1
    st, crcs = O.states_host(), O.crc_sum()
    for i, (f, l) in enumerate(zip(O.first, O.last)):
        if l >= f:  # the last extent's record is the object's state
            for fld in ("h", "x", "nx", "len"):
                assert ck[int(l)]["sha1"][fld].tolist() == st[i][fld].tolist(), (i, fld)
            assert int(ck[int(l)]["crc"]) == int(crcs[i])
    assert O.sha1_hex()[2] == hashlib.sha1(b"".join(bytes(host[a:a + n]) for a, n in ext9)).hexdigest()
    with pytest.raises(ValueError):
        batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, ctx=ctx).checkpoints_host()


# ---- 8. the text launch alone
def test_marshal_text_alone(env):
    """1 000 random records -- random h and x, nx negative, above 64 and in range, len up to 2^64 - 1, random crc
    and _pad words -- against the host codecs; the guard row behind the text untouched; n == 0 launches nothing."""
    torch, lib = env["torch"], env["lib"]
    rng = np.random.default_rng(1000)
    rec = np.zeros(1000, dtype=lib.CHECKPOINT_DTYPE)
    raw = rec.view(np.uint8).reshape(1000, REC)
    raw[:] = rng.integers(0, 256, size=raw.shape, dtype=np.uint8)  # every byte random, the _pad words too
    rec["sha1"]["nx"][:250] = rng.integers(-(1 << 62), 0, size=250)
    rec["sha1"]["nx"][250:500] = rng.integers(0, 65, size=250)
    rec["sha1"]["nx"][500:750] = rng.integers(65, 1 << 62, size=250)
    rec["sha1"]["len"][0], rec["sha1"]["len"][1], rec["sha1"]["nx"][2] = (1 << 64) - 1, 0, -1
    dev = torch.from_numpy(raw.reshape(-1).copy()).to("cuda:0")
    texts = device_texts(env, dev.data_ptr(), 1000)
    for i in range(1000):
        assert bytes(texts[i]) == host_text(lib, rec[i]), i
    assert bytes(texts[0][184:200]) == b"f" * 16 and bytes(texts[2][168:184]) == b"f" * 16
    out = torch.full((TEXT,), 0x7E, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    L = lib.lib()
    assert L.efes_checkpoints_marshal_text(env["ctx"].handle, dev.data_ptr(), 0, out.data_ptr(), None) == lib.EFES_OK
    assert L.efes_checkpoints_marshal_text(env["ctx"].handle, None, 0, None, None) == lib.EFES_OK
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x7E).all()


def test_arguments_on_the_device(env):
    """njobs == 0 returns EFES_OK and launches nothing; a NULL pointer array and the scratch errors of
    efes_hash_chain_mode are refused without a launch."""
    torch, lib, ctx = env["torch"], env["lib"], env["ctx"]
    L = lib.lib()
    C = CkptChains(env, [job(0, 100, INIT | FIN, 0, 0), job(100, 100, CHAIN | FIN, 0, 0)], [state_after(env, b"")], [0])
    j, p, s, nb = C.jobs.data_ptr(), C.ptrs.data_ptr(), C.scratch.data_ptr(), C.scratch_bytes
    for mode in (lib.MODE_DEEP, lib.MODE_GROUP[4]):
        assert L.efes_hash_chain_checkpoints(ctx.handle, None, 0, None, None, 0, None, mode) == lib.EFES_OK
        assert L.efes_hash_chain_checkpoints(ctx.handle, j, 0, p, s, nb, None, mode) == lib.EFES_OK
        assert L.efes_hash_chain_checkpoints(ctx.handle, j, 2, None, s, nb, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_checkpoints(ctx.handle, None, 2, p, s, nb, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_checkpoints(ctx.handle, j, 2, p, None, nb, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_checkpoints(ctx.handle, j, 2, p, s + 8, nb, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_checkpoints(ctx.handle, j, 2, p, s, nb - 1, None, mode) == lib.EFES_ERR_ARG
        assert L.efes_hash_chain_checkpoints(ctx.handle, j, lib.EFES_HASH_CHAIN_MAX_JOBS + 1, p, s, 1 << 40, None,
                                             mode) == lib.EFES_ERR_ARG
    assert L.efes_hash_chain_checkpoints(ctx.handle, j, 2, p, s, nb, None, lib.MODE_AUTO) == lib.EFES_ERR_ARG
    torch.cuda.synchronize()
    assert (C.status.cpu().numpy() == -99).all() and (C.records() == 0xA5).all(), "a refused call launched"
    C.run_ckpt(lib.MODE_DEEP)
    C.check()
    C.check_records()
