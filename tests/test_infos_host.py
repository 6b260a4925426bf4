"""Object infos on the host: efes_infos_marshal_text_host and efes_infos_unmarshal_text_host against the per-state
codecs of the library and against the oracle's MarshalText / UnmarshalText, bit for bit, over sentinel-guarded
outputs; every NULL-pointer variant the contract allows; texts spoiled at every field and word boundary with the
neighbours of the three hex ranges; and the stand-alone sanitizer program.  Needs no GPU."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from efes_amd._lib import EFES_ERR_INVALID_DIGEST, EFES_INFO_TEXT_BYTES, EFES_OK, EFES_SHA1_NX_REFUSED, SHA1_STATE_DTYPE, Crc32State, Infos, Sha1State

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = [0, 1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025]
# every field boundary (h|x at 40, x|nx at 168, nx|len at 184, len|crc at 200) and every kind of 8-character word boundary
POSITIONS = [0, 7, 8, 39, 40, 167, 168, 183, 184, 199, 200, 207]
# the neighbours of '0'-'9', 'A'-'F' and 'a'-'f', and the extremes
BYTES = [ord("g"), ord("G"), ord("/"), ord(":"), ord("@"), ord("`"), ord(" "), 0x00, 0x80, 0xFF]
SPOILS = list(itertools.product(POSITIONS, BYTES))
GUARD, SENTINEL = 64, 0xA5
T = EFES_INFO_TEXT_BYTES
# (sha1, crc32, status, counts) present or not: every combination the contract allows
VARIANTS = [v for v in itertools.product((True, False), repeat=4) if v[0] or v[1]]


def guarded(nbytes):
    """(whole, inner): a sentinel-filled buffer and the view of its nbytes in the middle, 8-byte aligned."""
    whole = np.full(nbytes + 2 * GUARD, SENTINEL, np.uint8)
    assert whole.ctypes.data % 8 == 0
    return whole, whole[GUARD:GUARD + nbytes]


def guards_intact(whole):
    return (whole[:GUARD] == SENTINEL).all() and (whole[-GUARD:] == SENTINEL).all()


def random_states(n, rng):
    """n states whose 104 bytes are all random (_pad and any nx included), and n random CRCs."""
    return rng.integers(0, 256, (n, 104), dtype=np.uint8), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)


def marshal_twin(L, states, crcs, sha1=True, crc32=True):
    n = len(crcs)
    whole, text = guarded(T * n)
    st, cr = np.ascontiguousarray(states), np.ascontiguousarray(crcs)
    req = Infos(text=text.ctypes.data if n else None, sha1=st.ctypes.data if sha1 and n else None,
                crc32=cr.ctypes.data if crc32 and n else None, status=0x4, counts=0x4, n=n)  # status and counts are ignored
    assert L.efes_infos_marshal_text_host(ctypes.byref(req)) == EFES_OK
    assert guards_intact(whole)
    return text.reshape(n, T).copy()


def unmarshal_twin(L, text, sha1=True, crc32=True, status=True, counts=True):
    """(states, crcs, status, counts) as the twin leaves them (None for an absent array), guards checked."""
    n = text.shape[0]
    flat = np.ascontiguousarray(text).reshape(-1)
    bufs = {k: guarded(size) for k, size in (("sha1", 104 * n), ("crc32", 4 * n), ("status", 4 * n), ("counts", 8))}
    on = dict(sha1=sha1, crc32=crc32, status=status, counts=counts)
    ptr = lambda k: bufs[k][1].ctypes.data if on[k] and (n or k == "counts") else None
    req = Infos(text=flat.ctypes.data if n else None, sha1=ptr("sha1"), crc32=ptr("crc32"), status=ptr("status"), counts=ptr("counts"), n=n)
    assert L.efes_infos_unmarshal_text_host(ctypes.byref(req)) == EFES_OK
    for k, (whole, inner) in bufs.items():
        assert guards_intact(whole), k
        if not on[k]:
            assert (inner == SENTINEL).all(), f"{k} is NULL and was written"
    return (bufs["sha1"][1].reshape(n, 104).copy() if sha1 else None, bufs["crc32"][1].view(np.uint32).copy() if crc32 else None,
            bufs["status"][1].view(np.int32).copy() if status else None, bufs["counts"][1].view(np.uint32).copy() if counts else None)


def codec_texts(L, states, crcs):
    """efes_sha1_state_marshal_text || efes_crc32_state_marshal_text per record."""
    out = np.zeros((len(crcs), T), np.uint8)
    a, b = ctypes.create_string_buffer(200), ctypes.create_string_buffer(8)
    for i in range(len(crcs)):
        L.efes_sha1_state_marshal_text(ctypes.byref(Sha1State.from_buffer_copy(states[i].tobytes())), a)
        L.efes_crc32_state_marshal_text(ctypes.byref(Crc32State(int(crcs[i]))), b)
        out[i] = np.frombuffer(a.raw + b.raw, np.uint8)
    return out


def oracle_texts(oracle, states, crcs):
    """oracle_sha1_marshal_text || oracle_crc32_marshal_text per record (the oracle's state has the same layout)."""
    out = np.zeros((len(crcs), T), np.uint8)
    d, c = oracle.Sha1(reset=False), oracle.Crc32()
    assert ctypes.sizeof(d.st) == 104
    for i in range(len(crcs)):
        ctypes.memmove(ctypes.byref(d.st), states[i].tobytes(), 104)
        c.st.crc = int(crcs[i])
        out[i] = np.frombuffer((d.marshal_text() + c.marshal_text()).encode(), np.uint8)
    return out


def oracle_verdicts(oracle, text):
    """Per record: oracle_sha1_unmarshal_text on 0..199 fails, or oracle_crc32_unmarshal_text on 200..207 fails."""
    d, c = oracle.Sha1(), oracle.Crc32()
    return np.array([d.unmarshal_text(bytes(r[:200])) != 0 or c.unmarshal_text(bytes(r[200:])) != 0 for r in text], dtype=bool)


def recase(text, rng):
    """Every letter's case chosen anew: a third of the records upper, a third lower, a third mixed per character."""
    out = text.copy()
    letters = (out >= ord("a")) & (out <= ord("f"))
    kind = rng.integers(0, 3, out.shape[0])[:, None]
    upper = letters & ((kind == 0) | ((kind == 2) & (rng.integers(0, 2, out.shape) == 1)))
    out[upper] -= 32
    return out


def spoil(text, rng, first_combo=0, records=None):
    """One character spoiled in each chosen record (records 0 and n - 1 among them): (spoiled text, chosen records).
    The (position, byte) pairs are taken from SPOILS in order, starting at first_combo."""
    n = text.shape[0]
    out = text.copy()
    if n == 0:
        return out, np.zeros(0, np.int64)
    if records is None:
        k = min(n, max(2, n // 8))
        records = np.unique(np.concatenate(([0, n - 1], rng.choice(n, k, replace=False))))
    for j, i in enumerate(records):
        pos, byte = SPOILS[(first_combo + j) % len(SPOILS)]
        out[i, pos] = byte
    return out, np.asarray(records)


def refusing_image():
    st = np.zeros(1, SHA1_STATE_DTYPE)
    st["nx"] = EFES_SHA1_NX_REFUSED
    return st.view(np.uint8).reshape(104)


def expected_states(states, bad):
    """What unmarshal leaves: the original with _pad 0, or the refusing image."""
    want = states.copy()
    want[:, 84:88] = 0
    want[bad] = refusing_image()
    return want


@pytest.fixture(scope="module")
def cases(efes_lib, oracle):
    """Per count: random states, their texts by the twin (checked in test_marshal_*), re-cased, spoiled, and the
    oracle's verdicts on the spoiled texts: made once and left unchanged."""
    L = efes_lib.lib()
    out = {}
    for n in COUNTS:
        rng = np.random.default_rng(1000 + n)
        states, crcs = random_states(n, rng)
        text = marshal_twin(L, states, crcs)
        cased = recase(text, rng)
        spoiled, chosen = spoil(cased, rng, first_combo=7 * n)
        out[n] = dict(states=states, crcs=crcs, text=text, cased=cased, spoiled=spoiled, chosen=chosen,
                      bad=oracle_verdicts(oracle, spoiled))
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_marshal_equals_the_codecs_and_the_oracle(efes_lib, oracle, cases, n):
    c = cases[n]
    assert (c["text"] == codec_texts(efes_lib.lib(), c["states"], c["crcs"])).all()
    assert (c["text"] == oracle_texts(oracle, c["states"], c["crcs"])).all()
    lower = ((c["text"] >= ord("0")) & (c["text"] <= ord("9"))) | ((c["text"] >= ord("a")) & (c["text"] <= ord("f")))
    assert lower.all(), "lower-case hex only"


@pytest.mark.parametrize("n", COUNTS)
def test_marshal_without_one_digest(efes_lib, cases, n):
    L, c = efes_lib.lib(), cases[n]
    no_sha = marshal_twin(L, c["states"], c["crcs"], sha1=n == 0)
    no_crc = marshal_twin(L, c["states"], c["crcs"], crc32=n == 0)
    if n:
        assert (no_sha[:, :200] == ord("0")).all() and (no_sha[:, 200:] == c["text"][:, 200:]).all()
        assert (no_crc[:, 200:] == ord("0")).all() and (no_crc[:, :200] == c["text"][:, :200]).all()


def test_a_refusing_state_marshals_like_any_other(efes_lib, oracle):
    st = refusing_image()[None, :]
    crc = np.zeros(1, np.uint32)
    text = marshal_twin(efes_lib.lib(), st, crc)
    assert (text == oracle_texts(oracle, st, crc)).all()
    assert bytes(text[0, 168:184]) == b"%016x" % EFES_SHA1_NX_REFUSED


@pytest.mark.parametrize("n", COUNTS)
def test_unmarshal_of_recased_texts(efes_lib, oracle, cases, n):
    L, c = efes_lib.lib(), cases[n]
    assert not oracle_verdicts(oracle, c["cased"]).any()
    if n >= 3:
        assert (c["cased"] != c["text"]).any() and ((c["cased"] >= ord("a")) & (c["cased"] <= ord("f"))).any()
    states, crcs, status, counts = unmarshal_twin(L, c["cased"])
    assert (states == expected_states(c["states"], np.zeros(n, bool))).all()
    assert (states[:, 84:88] == 0).all(), "_pad is written as 0"
    assert (crcs == c["crcs"]).all() and (status == EFES_OK).all() and counts.tolist() == [n, 0]
    # against the per-state codec of the library, nx stored as decoded whatever its value
    s, k = Sha1State(), Crc32State()
    for i in range(min(n, 40)):
        assert L.efes_sha1_state_unmarshal_text(ctypes.byref(s), bytes(c["cased"][i, :200]), 200) == EFES_OK
        assert L.efes_crc32_state_unmarshal_text(ctypes.byref(k), bytes(c["cased"][i, 200:]), 8) == EFES_OK
        got = states[i].view(SHA1_STATE_DTYPE)[0]
        assert (list(s.h), bytes(s.x), s.nx, s.len, k.crc) == (got["h"].tolist(), bytes(got["x"]), int(got["nx"]), int(got["len"]), int(crcs[i]))


@pytest.mark.parametrize("n", COUNTS)
def test_unmarshal_of_spoiled_texts_in_every_variant(efes_lib, cases, n):
    L, c = efes_lib.lib(), cases[n]
    bad = c["bad"]
    assert bad.sum() == len(c["chosen"]) and bad[c["chosen"]].all(), "the oracle refuses exactly the spoiled records"
    if n:
        assert bad[0] and bad[n - 1]
    want = expected_states(c["states"], bad)
    want_crcs = np.where(bad, 0, c["crcs"]).astype(np.uint32)
    for sha1, crc32, status, counts in VARIANTS:
        got = unmarshal_twin(L, c["spoiled"], sha1, crc32, status, counts)
        if sha1:
            assert (got[0] == want).all(), "invalid records hold exactly the refusing image, valid ones their state"
        if crc32:
            assert (got[1] == want_crcs).all()
        if status:
            assert (got[2] == np.where(bad, EFES_ERR_INVALID_DIGEST, EFES_OK)).all()
        if counts:
            assert got[3].tolist() == [n - int(bad.sum()), int(bad.sum())]


def test_every_position_with_every_byte(efes_lib, oracle):
    """All 120 (position, byte) pairs at once, one per record, records 0 and n - 1 among them."""
    L, n = efes_lib.lib(), 257
    rng = np.random.default_rng(5)
    states, crcs = random_states(n, rng)
    text = recase(marshal_twin(L, states, crcs), rng)
    records = np.unique(np.concatenate(([0, n - 1], rng.choice(np.arange(1, n - 1), len(SPOILS) - 2, replace=False))))
    assert len(records) == len(SPOILS)
    spoiled, chosen = spoil(text, rng, records=records)
    assert sorted((int(p), int(spoiled[i, p])) for i in chosen for p in np.nonzero(spoiled[i] != text[i])[0]) == sorted(SPOILS)
    bad = oracle_verdicts(oracle, spoiled)
    assert bad.sum() == len(SPOILS) and bad[chosen].all()
    got = unmarshal_twin(L, spoiled)
    assert (got[0] == expected_states(states, bad)).all() and (got[1] == np.where(bad, 0, crcs)).all()
    assert (got[2] == np.where(bad, EFES_ERR_INVALID_DIGEST, EFES_OK)).all() and got[3].tolist() == [n - len(SPOILS), len(SPOILS)]
    # every word of every state is written by every call: nothing of an earlier call's states survives a second one
    again = unmarshal_twin(L, text)
    assert (again[0] == expected_states(states, np.zeros(n, bool))).all() and again[3].tolist() == [n, 0]


def test_a_spoiled_crc_text_refuses_a_sha1_only_table_and_the_other_way_round(efes_lib):
    """All 208 characters are checked even when sha1 or crc32 is NULL: an `.info` record always holds both."""
    L = efes_lib.lib()
    rng = np.random.default_rng(9)
    states, crcs = random_states(4, rng)
    text = marshal_twin(L, states, crcs)
    text[1, 203] = ord("x")  # in the CRC's characters
    text[2, 100] = ord("x")  # in the SHA-1 state's
    sha_only = unmarshal_twin(L, text, crc32=False)
    assert sha_only[2].tolist() == [0, EFES_ERR_INVALID_DIGEST, EFES_ERR_INVALID_DIGEST, 0] and sha_only[3].tolist() == [2, 2]
    assert (sha_only[0][1] == refusing_image()).all() and (sha_only[0][2] == refusing_image()).all()
    crc_only = unmarshal_twin(L, text, sha1=False)
    assert crc_only[2].tolist() == [0, EFES_ERR_INVALID_DIGEST, EFES_ERR_INVALID_DIGEST, 0]
    assert crc_only[1].tolist() == [int(crcs[0]), 0, 0, int(crcs[3])], "a CRC-only table has no refusing state: the CRC is 0"


def test_standalone_sanitizer_program(tmp_path):
    """tests/cpp/infos_invalid.cpp runs the twins on heap arrays of exact size, text at an odd address, first and
    last records spoiled, built with -fsanitize=address,undefined together with efes_infos.cpp and the shared rules:
    an out-of-range read or write ends it with a report.  A program of its own with the sanitizer runtimes linked in
    statically: it needs nothing preloaded and runs in the environment it is given, unchanged."""
    exe = tmp_path / "infos_invalid"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "infos_invalid.cpp"),
           os.path.join(ROOT, "efes_amd", "csrc", "efes_infos.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    missing = [line for line in built.stderr.splitlines() if "cannot find" in line and ("asan" in line or "ubsan" in line)]
    if built.returncode != 0 and missing:
        pytest.skip("the toolchain lacks the static sanitizer runtime: " + missing[0].strip())
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-4000:]
    assert "records ok" in ran.stdout
