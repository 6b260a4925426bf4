"""GPU parity of efes_infos_unmarshal_text and efes_infos_marshal_text: the device calls against their host twins,
byte for byte, over guarded device outputs at the kernels' seams (two records per wavefront, 32 per workgroup);
two PATCH rounds of 65 objects through texts, each round queued on one stream with no host synchronisation between
unmarshal, builder, walk, results and marshal, against hashlib, zlib and the oracle's replay; the same set with
three texts spoiled; and a CRC-only set resumed from texts.  Bit-exact."""
import ctypes
import hashlib
import zlib

import numpy as np
import pytest

from test_infos_host import (GUARD, SENTINEL, T, VARIANTS, expected_states, marshal_twin, oracle_texts, random_states, recase,
                             spoil, unmarshal_twin)

pytestmark = pytest.mark.gpu

BUF_BYTES = 1 << 20
SEAMS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025]
NOBJECTS = 65  # one wavefront of the wide walk plus one lane
ROUND1 = [0, 1, 55, 56, 63, 64, 65, 119, 128, 1000, 4113]  # nx at the cut: 0, 1, 55, 56, 63, 0, 1, 55, 0, 40, 17
ROUND2 = [0, 1, 8, 9, 63, 64, 65, 200, 4096]
SPOILED = [0, 31, 64]


@pytest.fixture(scope="module")
def env():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from efes_amd import _lib, batch, hashing
    ctx = hashing.default_context(0)
    buf = torch.empty(BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    ctx.fill_synthetic(buf.data_ptr(), BUF_BYTES, 0x1F05, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(torch=torch, hashing=hashing, batch=batch, lib=_lib, ctx=ctx, buf=buf, host=buf.cpu().numpy())


# ---- the device calls against the twins
class DeviceGuarded:
    """nbytes of device memory between two sentinel-filled guards; body() and guards_intact() after fetch()."""

    def __init__(self, torch, nbytes, fill=None):
        image = np.full(nbytes + 2 * GUARD, SENTINEL, np.uint8)
        if fill is not None:
            image[GUARD:GUARD + nbytes] = np.ascontiguousarray(fill).view(np.uint8).reshape(-1)
        self.nbytes, self.t = nbytes, torch.from_numpy(image).to("cuda:0")
        assert self.t.data_ptr() % 8 == 0

    @property
    def ptr(self):
        return self.t.data_ptr() + GUARD

    def fetch(self):
        self.host = self.t.cpu().numpy()
        return self

    def body(self):
        return self.host[GUARD:GUARD + self.nbytes]

    def guards_intact(self):
        return (self.host[:GUARD] == SENTINEL).all() and (self.host[-GUARD:] == SENTINEL).all()


def device_unmarshal(env, text, sha1=True, crc32=True, status=True, counts=True):
    """efes_infos_unmarshal_text over guarded device outputs: the tuple unmarshal_twin returns."""
    torch, L = env["torch"], env["lib"]
    n = text.shape[0]
    text_d = DeviceGuarded(torch, T * n, text)
    on = dict(sha1=sha1, crc32=crc32, status=status, counts=counts)
    bufs = {k: DeviceGuarded(torch, size) for k, size in (("sha1", 104 * n), ("crc32", 4 * n), ("status", 4 * n), ("counts", 8))}
    req = L.Infos(text=text_d.ptr, n=n, **{k: bufs[k].ptr if on[k] else None for k in bufs})
    torch.cuda.synchronize()  # the sentinels and the texts are in place
    assert L.lib().efes_infos_unmarshal_text(env["ctx"].handle, ctypes.byref(req), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert (text_d.fetch().body().reshape(n, T) == text).all() and text_d.guards_intact(), "the texts are only read"
    for k, g in bufs.items():
        assert g.fetch().guards_intact(), k
        if not on[k]:
            assert (g.body() == SENTINEL).all(), f"{k} is NULL and was written"
    return (bufs["sha1"].body().reshape(n, 104) if sha1 else None, bufs["crc32"].body().view(np.uint32) if crc32 else None,
            bufs["status"].body().view(np.int32) if status else None, bufs["counts"].body().view(np.uint32) if counts else None)


def device_marshal(env, states, crcs, sha1=True, crc32=True):
    torch, L = env["torch"], env["lib"]
    n = len(crcs)
    st, cr, out = DeviceGuarded(torch, 104 * n, states), DeviceGuarded(torch, 4 * n, crcs), DeviceGuarded(torch, T * n)
    req = L.Infos(text=out.ptr, sha1=st.ptr if sha1 else None, crc32=cr.ptr if crc32 else None, status=0x4, counts=0x4, n=n)
    torch.cuda.synchronize()
    assert L.lib().efes_infos_marshal_text(env["ctx"].handle, ctypes.byref(req), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert out.fetch().guards_intact() and (st.fetch().body() == np.ascontiguousarray(states).reshape(-1)).all()
    return out.body().reshape(n, T)


@pytest.fixture(scope="module")
def inputs(efes_lib):
    """Per seam count: random states, their texts re-cased, and those with about one record in eight spoiled (records
    0 and n - 1 among them) at the positions and with the bytes of test_infos_host; made once, left unchanged."""
    L, out = efes_lib.lib(), {}
    for n in SEAMS:
        rng = np.random.default_rng(2000 + n)
        states, crcs = random_states(n, rng)
        cased = recase(marshal_twin(L, states, crcs), rng)
        spoiled, chosen = spoil(cased, rng, first_combo=11 * n)
        out[n] = dict(states=states, crcs=crcs, cased=cased, spoiled=spoiled, chosen=chosen)
    return out


@pytest.mark.parametrize("n", SEAMS)
def test_unmarshal_equals_the_twin(env, efes_lib, inputs, n):
    L, c = efes_lib.lib(), inputs[n]
    for which in ("cased", "spoiled"):
        for variant in VARIANTS:
            got, want = device_unmarshal(env, c[which], *variant), unmarshal_twin(L, c[which], *variant)
            for g, w, name in zip(got, want, ("sha1", "crc32", "status", "counts")):
                assert (g is None) == (w is None) and (g is None or g.tobytes() == w.tobytes()), (n, which, variant, name)
    # and what the twin's own tests pin down, once more on the device's bytes
    states, crcs, status, counts = device_unmarshal(env, c["spoiled"])
    bad = np.zeros(n, bool)
    bad[c["chosen"]] = True
    assert (states == expected_states(c["states"], bad)).all() and (crcs == np.where(bad, 0, c["crcs"])).all()
    assert (status == np.where(bad, env["lib"].EFES_ERR_INVALID_DIGEST, 0)).all() and counts.tolist() == [n - int(bad.sum()), int(bad.sum())]


@pytest.mark.parametrize("n", SEAMS)
def test_marshal_equals_the_twin_and_the_checkpoint_texts(env, efes_lib, inputs, n):
    L, c = efes_lib.lib(), inputs[n]
    torch = env["torch"]
    for sha1, crc32 in ((True, True), (True, False), (False, True)):
        got, want = device_marshal(env, c["states"], c["crcs"], sha1, crc32), marshal_twin(L, c["states"], c["crcs"], sha1, crc32)
        assert got.tobytes() == want.tobytes(), (n, sha1, crc32)
    # efes_checkpoints_marshal_text over the same states packed into 112-byte records
    rec = np.zeros(n, efes_lib.CHECKPOINT_DTYPE)
    rec.view(np.uint8).reshape(n, 112)[:, :104] = c["states"]
    rec["crc"] = c["crcs"]
    rec_d = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to("cuda:0")
    text_d = torch.zeros(T * n, dtype=torch.uint8, device="cuda:0")
    env["ctx"].checkpoints_marshal_text(rec_d.data_ptr(), n, text_d.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert text_d.cpu().numpy().tobytes() == device_marshal(env, c["states"], c["crcs"]).tobytes()


def test_no_records(env):
    """n == 0: EFES_OK, counts written whole, nothing else launched; marshal does nothing."""
    torch, L = env["torch"], env["lib"]
    counts = DeviceGuarded(torch, 8)
    req = L.Infos(counts=counts.ptr, n=0)
    torch.cuda.synchronize()
    assert L.lib().efes_infos_unmarshal_text(env["ctx"].handle, ctypes.byref(req), None) == 0
    assert L.lib().efes_infos_marshal_text(env["ctx"].handle, ctypes.byref(req), None) == 0
    env["ctx"].sync()
    assert counts.fetch().body().view(np.uint32).tolist() == [0, 0] and counts.guards_intact()


# ---- two PATCH rounds through texts
def rounds(seed=77):
    """(round 1, round 2): per object its extents (offset, length) in the 1 MiB buffer, at any alignment."""
    rng = np.random.default_rng(seed)
    one = [[(int(rng.integers(0, BUF_BYTES - 8192)), ROUND1[i % len(ROUND1)])] for i in range(NOBJECTS)]
    two = [[(int(rng.integers(0, BUF_BYTES - 8192)), ROUND2[int(rng.integers(0, len(ROUND2)))]) for _ in range(1 + (i + i // 3) % 3)]
           for i in range(NOBJECTS)]
    two[0][0], two[31][0] = (two[0][0][0], 0), (two[31][0][0], 64)  # a refused object's first Write may be empty
    return one, two


def whole(host, *parts):
    return b"".join(host[o:o + n].tobytes() for obj in parts for o, n in obj)


@pytest.fixture(scope="module")
def reference(env, oracle):
    """For the 65 objects: hashlib's and zlib's digests of the whole objects, and the oracle replaying Write(part 1),
    MarshalText, UnmarshalText, then a Write per extent of round 2 -- the states with their stale x bytes, and the
    texts after either round.  Computed once."""
    host = env["host"]
    one, two = rounds()
    expected = np.zeros((NOBJECTS, 24), np.uint8)
    states = np.zeros(NOBJECTS, env["lib"].SHA1_STATE_DTYPE)
    texts1, texts2 = [], []
    for i in range(NOBJECTS):
        data = whole(host, one[i], two[i])
        expected[i] = np.frombuffer(hashlib.sha1(data).digest() + zlib.crc32(data).to_bytes(4, "big"), np.uint8)
        d, c = oracle.Sha1(), oracle.Crc32()
        assert d.write(whole(host, one[i])) == 0
        c.write(whole(host, one[i]))
        texts1.append((d.marshal_text().encode(), c.marshal_text().encode()))
        d2, c2 = oracle.Sha1(reset=False), oracle.Crc32()
        assert d2.unmarshal_text(texts1[-1][0]) == 0 and c2.unmarshal_text(texts1[-1][1]) == 0
        for o, n in two[i]:
            assert d2.write(host[o:o + n]) == 0
            c2.write(host[o:o + n])
        assert d2.hexdigest() == bytes(expected[i, :20]).hex() and c2.sum32() == zlib.crc32(data)
        states[i] = (d2.h, list(d2.x), 0, d2.nx, d2.length)
        texts2.append((d2.marshal_text().encode(), c2.marshal_text().encode()))
    return dict(one=one, two=two, expected=expected, states=states, texts1=texts1, texts2=texts2)


def walks(lib):
    return {"chain": None, "group16": lib.MODE_GROUP[16], "wide": "wide"}


def two_rounds(env, ref, walk, spoiled=(), **kw):
    """Both rounds on a side stream; every call of a round is queued behind the one before it and the host waits only
    once, at the end.  Round 1 is a fresh set; its info_texts(device=True), with the texts of `spoiled` objects broken
    on the device, is round 2's infos=.  Returns (round 1, round 2, records, counts, bad, texts after round 2)."""
    torch, batch = env["torch"], env["batch"]
    exp_d = torch.from_numpy(ref["expected"].copy()).to("cuda:0")  # on the device before anything is queued
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r1 = batch.DeviceObjects(env["buf"].data_ptr(), ref["one"], ctx=env["ctx"], sha1=True, walk=walk, build="device")
        r1.submit()
        texts = r1.info_texts(device=True)
        for k, i in enumerate(spoiled):  # in stream order behind the marshal
            texts[T * i + (0, 199, 207)[k % 3]] = (ord("g"), 0x80, ord(" "))[k % 3]
        r2 = batch.DeviceObjects(env["buf"].data_ptr(), ref["two"], ctx=env["ctx"], sha1=True, walk=walk, build="device", infos=texts, **kw)
        r2.submit()
        rec_d = r2._results_call(exp_d, 3, records=True)
        after = r2.info_texts(device=True)
    torch.cuda.synchronize()  # the one wait
    counts, bad = r2._results_fetch()
    rec = rec_d.cpu().numpy()[: NOBJECTS * 32].view(env["lib"].OBJECT_RESULT_DTYPE)
    return r1, r2, rec, counts, bad, after.cpu().numpy().reshape(NOBJECTS, T)


@pytest.mark.parametrize("walk", ["chain", "group16", "wide"])
def test_two_patch_rounds_in_stream_order(env, oracle, reference, walk):
    L, ref = env["lib"], reference
    r1, r2, rec, counts, bad, after = two_rounds(env, ref, walks(L)[walk])
    assert (r1.status_host() == 0).all() and (r2.status_host() == 0).all()
    assert r1.info_texts() == ref["texts1"]
    assert r2.resume_counts() == (NOBJECTS, 0) and (r2.resume_status_host() == 0).all()
    assert r2.sha1_hex() == [bytes(e[:20]).hex() for e in ref["expected"]], "hashlib.sha1 of each whole object"
    assert r2.crc_sum().tolist() == [int.from_bytes(bytes(e[20:]), "big") for e in ref["expected"]], "zlib.crc32"
    got, want = r2.states_host(), ref["states"]
    for f in ("h", "x", "nx", "len"):  # x with its stale bytes
        assert (got[f] == want[f]).all(), (walk, f)
    assert [(bytes(r[:200]), bytes(r[200:])) for r in after] == ref["texts2"] == r2.info_texts()
    assert counts.tolist() == [NOBJECTS, 0, 0, 0] and bad.size == 0
    assert (rec["sum"] == ref["expected"]).all() and (rec["verdict"] == L.EFES_VERDICT_OK).all()
    # reset() restores the decoded states without decoding again
    r2.reset()
    r2.run()
    assert r2.info_texts() == ref["texts2"]


@pytest.mark.parametrize("walk", ["chain", "group16", "wide"])
def test_three_spoiled_texts_are_refused(env, reference, walk):
    L, ref = env["lib"], reference
    r1, r2, rec, counts, bad, after = two_rounds(env, ref, walks(L)[walk], spoiled=SPOILED)
    ok = np.ones(NOBJECTS, bool)
    ok[SPOILED] = False
    assert bad.tolist() == SPOILED and counts.tolist() == [NOBJECTS - 3, 0, 3, 0]
    assert (rec["verdict"][~ok] == L.EFES_VERDICT_FAILED).all() and (rec["status"][~ok] == L.EFES_ERR_STATE).all()
    assert (rec["sum"][~ok] == 0).all()
    assert (rec["verdict"][ok] == L.EFES_VERDICT_OK).all() and (rec["status"][ok] == 0).all() and (rec["sum"][ok] == ref["expected"][ok]).all()
    assert r2.resume_counts() == (NOBJECTS - 3, 3)
    assert r2.resume_status_host().tolist() == [0 if k else L.EFES_ERR_INVALID_DIGEST for k in ok]
    status = r2.status_host()
    for i, (f, l) in enumerate(zip(r2.first, r2.last)):  # every Write into the refusing state, and only those
        assert (status[f:l + 1] == (0 if ok[i] else L.EFES_ERR_STATE)).all(), i
    states = r2.states_host()
    assert (states["nx"][~ok] == L.EFES_SHA1_NX_REFUSED).all() and (states["h"][~ok] == 0).all() and (states["len"][~ok] == 0).all()
    assert [(bytes(r[:200]), bytes(r[200:])) for r, k in zip(after, ok) if k] == [t for t, k in zip(ref["texts2"], ok) if k]


def test_refused_objects_are_not_gathered(env, reference):
    """walk="wide" with copy_to=: the destination keeps its sentinel over the three refused objects' ranges and holds
    the source bytes everywhere else."""
    torch, L, ref = env["torch"], env["lib"], reference
    _, room = env["batch"].default_copy_offsets(ref["two"])
    dest = torch.full((room + 512,), 0xEE, dtype=torch.uint8, device="cuda:0")
    r1, r2, rec, counts, bad, after = two_rounds(env, ref, "wide", spoiled=SPOILED, copy_to=dest.data_ptr() + 256)
    assert bad.tolist() == SPOILED and counts.tolist() == [NOBJECTS - 3, 0, 3, 0]
    image = np.full(room + 512, 0xEE, np.uint8)
    for i, (obj, at) in enumerate(zip(ref["two"], r2.copy_offsets.tolist())):
        if i not in SPOILED:
            data = np.frombuffer(whole(env["host"], obj), np.uint8)
            image[256 + at:256 + at + data.size] = data
    landed = dest.cpu().numpy()
    assert (landed == image).all(), np.nonzero(landed != image)[0][:8]
    assert sum(n for i in SPOILED for _, n in ref["two"][i]) > 0, "the refused objects have bytes that were not gathered"


def test_a_crc_only_set_resumed_from_texts(env, reference):
    """The CRCs of the whole objects equal zlib's.  A CRC-only table has no refusing state: with one text spoiled
    resume_status_host() names it, and its CRC state started from 0 -- so it holds zlib's CRC of round 2's bytes
    alone, which is why such a caller reads the statuses or counts before it trusts the CRCs."""
    torch, batch, L, ref, host = env["torch"], env["batch"], env["lib"], reference, env["host"]
    r1 = batch.DeviceObjects(env["buf"].data_ptr(), ref["one"], ctx=env["ctx"], build="device")
    r1.submit()
    texts = r1.info_texts(device=True)
    r2 = batch.DeviceObjects(env["buf"].data_ptr(), ref["two"], ctx=env["ctx"], build="device", infos=texts)
    r2.submit()
    torch.cuda.synchronize()
    assert [t[0] for t in r1.info_texts()] == [b"0" * 200] * NOBJECTS, "a set without SHA-1 marshals it as zeros"
    assert [t[1] for t in r1.info_texts()] == [t[1] for t in ref["texts1"]]
    want = [int.from_bytes(bytes(e[20:]), "big") for e in ref["expected"]]
    assert r2.crc_sum().tolist() == want and r2.resume_counts() == (NOBJECTS, 0)
    assert [t[1] for t in r2.info_texts()] == [t[1] for t in ref["texts2"]]
    victim = 40
    texts[T * victim + 100] = ord("G")  # among the SHA-1 state's characters, which this set does not keep: all 208 count
    r3 = batch.DeviceObjects(env["buf"].data_ptr(), ref["two"], ctx=env["ctx"], build="device", infos=texts)
    r3.run()
    status = r3.resume_status_host()
    assert np.nonzero(status)[0].tolist() == [victim] and status[victim] == L.EFES_ERR_INVALID_DIGEST and r3.resume_counts() == (NOBJECTS - 1, 1)
    assert (r3.status_host() == 0).all(), "nothing refuses the Writes of a CRC-only object"
    want[victim] = zlib.crc32(whole(host, ref["two"][victim]))  # from 0
    assert r3.crc_sum().tolist() == want


@pytest.mark.parametrize("build", ["host", "device", "from_table"])
def test_infos_as_host_array_and_as_pairs(env, reference, build):
    """infos= as a host (nobjects, 208) array and as a list of pairs, one of them of the wrong length: that object is
    refused and the others run; through each way of building the set."""
    torch, batch, L, ref = env["torch"], env["batch"], env["lib"], reference
    pairs = list(ref["texts1"])
    pairs[5] = (pairs[5][0][:199], pairs[5][1])
    rows = np.stack([np.frombuffer(a + b, np.uint8) for a, b in ref["texts1"]])
    for infos, refused in ((rows, []), (pairs, [5])):
        if build == "from_table":
            from test_objects_jobs_host import table_of
            ext, first = table_of(ref["two"])
            up = lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view)).to("cuda:0")
            O = batch.DeviceObjects.from_table(env["buf"].data_ptr(), up(ext, np.int64), up(first, np.int32), ctx=env["ctx"], sha1=True,
                                               walk="wide", infos=infos)
        else:
            O = batch.DeviceObjects(env["buf"].data_ptr(), ref["two"], ctx=env["ctx"], sha1=True, walk="wide", build=build, infos=infos)
        O.submit()
        rec, counts, bad = O.results(ref["expected"])
        assert bad.tolist() == refused and counts.tolist() == [NOBJECTS - len(refused), 0, len(refused), 0], build
        assert O.resume_counts() == (NOBJECTS - len(refused), len(refused))
        ok = np.ones(NOBJECTS, bool)
        ok[refused] = False
        assert (rec["sum"][ok] == ref["expected"][ok]).all()
