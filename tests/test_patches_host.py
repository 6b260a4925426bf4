"""PATCH logs on the host: efes_patches_table_host against the normative automaton, restated here in Python, over
sentinel-guarded outputs: the receiver's test scripts (tests/golden/patches_scripts.json), restarts, PATCHes behind a
DONE, INVALID records, uploads without a PATCH, offsets == NULL, arithmetic at 2^64, seeded random logs whose verdict
shares are asserted, round equivalence (the DEFERRED PATCHes resubmitted log after log give what a plain sequential
replay gives), and the stand-alone sanitizer program.  Needs no GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from efes_amd._lib import (EFES_OK, EFES_PATCH_ADMITTED, EFES_PATCH_CONFLICT, EFES_PATCH_DEFERRED, EFES_PATCH_DONE, EFES_PATCH_INVALID,
                           EFES_PATCH_LENGTH_UNKNOWN, EFES_PATCH_OBJ_DEFERRED, EFES_PATCH_OBJ_DONE, EFES_PATCH_OBJ_RESTARTED, EXTENT_DTYPE,
                           PATCH_ANSWER_DTYPE, PATCH_DTYPE, PATCH_OBJECT_DTYPE, SHA1_STATE_DTYPE, Patches)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL = 64, 0xA5
MASK = (1 << 64) - 1
UNKNOWN = EFES_PATCH_LENGTH_UNKNOWN
VERDICTS = dict(ADMITTED=EFES_PATCH_ADMITTED, CONFLICT=EFES_PATCH_CONFLICT, DEFERRED=EFES_PATCH_DEFERRED, DONE=EFES_PATCH_DONE,
                INVALID=EFES_PATCH_INVALID)
OUTPUTS = ("extents", "first", "answers", "objects", "patch_of", "counts")
OPTIONAL = ("answers", "objects", "patch_of", "counts")
RANDOM_SHAPES = [(64, 1025), (257, 4096), (1000, 1023), (5000, 20000), (65537, 70000)]


def make_log(records):
    """A PATCH_DTYPE array of (object, file_offset, length, file_length[, data_offset]) tuples; bodies lie one behind the
    other where no data_offset is given."""
    log = np.zeros(len(records), PATCH_DTYPE)
    at = 0
    for a, r in enumerate(records):
        log[a]["object"], log[a]["file_offset"], log[a]["length"], log[a]["file_length"] = r[0], r[1] & MASK, r[2] & MASK, r[3] & MASK
        log[a]["data_offset"] = r[4] if len(r) > 4 else at
        at += int(r[2]) if len(r) <= 4 else 0
    return log


def fresh_state_image():
    st = np.zeros(1, SHA1_STATE_DTYPE)
    st["h"] = [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
    return st.view(np.uint8).reshape(104).copy()


def automaton(log, offsets, m):
    """The issue's rules, word for word: every output of the call as numpy arrays, and `restarted` per object."""
    n = len(log)
    cur = [0] * m if offsets is None else [int(x) for x in offsets]
    acc, closed, restarted, deferred, done = ([False] * m for _ in range(5))
    admitted = [0] * m
    obj = log["object"].astype(np.int64)
    key = np.minimum(obj, m - 1) if m else obj
    patch_of = np.argsort(key, kind="stable").astype(np.uint32)
    slot = np.empty(n, np.uint32)
    slot[patch_of] = np.arange(n, dtype=np.uint32)
    first = np.searchsorted(key[patch_of], np.arange(m + 1)).astype(np.uint32) if n else np.zeros(m + 1, np.uint32)
    first[m] = n
    answers = np.zeros(n, PATCH_ANSWER_DTYPE)
    extents = np.zeros(n, EXTENT_DTYPE)
    counts = np.zeros(5, np.uint32)
    fo_, len_, fl_, do_ = (log[k].tolist() for k in ("file_offset", "length", "file_length", "data_offset"))
    for a in range(n):
        i = int(obj[a])

        def answer(verdict, offset):
            answers[a] = (offset, verdict, slot[a])
            counts[verdict] += 1
            if verdict in (EFES_PATCH_ADMITTED, EFES_PATCH_DONE):
                extents[slot[a]] = (do_[a], len_[a])

        if i >= m:
            answer(EFES_PATCH_INVALID, 0)
            continue
        if closed[i]:
            deferred[i] = True
            answer(EFES_PATCH_DEFERRED, cur[i])
            continue
        if fo_[a] == 0:
            if acc[i]:
                closed[i] = deferred[i] = True
                answer(EFES_PATCH_DEFERRED, cur[i])
                continue
            restarted[i] = True
            cur[i] = len_[a]
        elif fo_[a] == cur[i]:
            cur[i] = (cur[i] + len_[a]) & MASK
        else:
            answer(EFES_PATCH_CONFLICT, cur[i])
            continue
        acc[i] = True
        admitted[i] += 1
        if cur[i] == fl_[a]:
            closed[i] = done[i] = True
            answer(EFES_PATCH_DONE, cur[i])
        else:
            answer(EFES_PATCH_ADMITTED, cur[i])
    objects = np.zeros(m, PATCH_OBJECT_DTYPE)
    objects["offset"] = np.array(cur, dtype=np.uint64)
    objects["flags"] = (np.array(restarted, dtype=np.uint32) * EFES_PATCH_OBJ_RESTARTED + np.array(done, dtype=np.uint32) * EFES_PATCH_OBJ_DONE +
                        np.array(deferred, dtype=np.uint32) * EFES_PATCH_OBJ_DEFERRED) if m else 0
    objects["admitted"] = np.array(admitted, dtype=np.uint32)
    return dict(extents=extents, first=first, answers=answers, objects=objects, patch_of=patch_of, counts=counts,
                restarted=np.array(restarted, dtype=bool))


def random_states(m, rng):
    return rng.integers(0, 256, (m, 104), dtype=np.uint8), rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(np.uint32)


def expected_states(states, crcs, restarted):
    want_s, want_c = states.copy(), crcs.copy()
    want_s[restarted] = fresh_state_image()
    want_c[restarted] = 0
    return want_s, want_c


def output_sizes(m, n):
    return dict(extents=16 * n, first=4 * (m + 1), answers=16 * n, objects=16 * m, patch_of=4 * n, counts=20)


def views(raw):
    """The byte bodies of the outputs as the typed arrays automaton() returns."""
    return dict(extents=raw["extents"].view(EXTENT_DTYPE), first=raw["first"].view(np.uint32), answers=raw["answers"].view(PATCH_ANSWER_DTYPE),
                objects=raw["objects"].view(PATCH_OBJECT_DTYPE), patch_of=raw["patch_of"].view(np.uint32), counts=raw["counts"].view(np.uint32))


def guarded(nbytes):
    whole = np.full(nbytes + 2 * GUARD, SENTINEL, np.uint8)
    assert whole.ctypes.data % 8 == 0
    return whole, whole[GUARD:GUARD + nbytes]


def twin(L, log, offsets, m, states=None, crcs=None, drop=()):
    """efes_patches_table_host over guarded outputs: the typed outputs (None for a dropped one) and the states after."""
    n = len(log)
    log = np.ascontiguousarray(log)
    offs = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
    bufs = {k: guarded(size) for k, size in output_sizes(m, n).items()}
    st = None if states is None else guarded(104 * m)
    cr = None if crcs is None else guarded(4 * m)
    if st:
        st[1][:] = states.reshape(-1)
    if cr:
        cr[1][:] = crcs.view(np.uint8)
    ptr = lambda k: None if k in drop else bufs[k][1].ctypes.data if bufs[k][1].size else bufs[k][0].ctypes.data + GUARD
    req = Patches(log=log.ctypes.data if n else None, offsets=None if offs is None or m == 0 else offs.ctypes.data,
                  sha1=st[0].ctypes.data + GUARD if st else None, crc32=cr[0].ctypes.data + GUARD if cr else None, nobjects=m, npatches=n,
                  **{k: ptr(k) for k in OUTPUTS})
    assert L.efes_patches_table_host(ctypes.byref(req)) == EFES_OK
    for k, (whole, inner) in list(bufs.items()) + [(k, v) for k, v in (("sha1", st), ("crc32", cr)) if v]:
        assert (whole[:GUARD] == SENTINEL).all() and (whole[-GUARD:] == SENTINEL).all(), f"{k}: a guard was written"
        if k in drop:
            assert (inner == SENTINEL).all(), f"{k} is NULL and was written"
    got = views({k: bufs[k][1].copy() for k in OUTPUTS})
    for k in drop:
        got[k] = None
    got["sha1"] = st[1].reshape(m, 104).copy() if st else None
    got["crc32"] = cr[1].view(np.uint32).copy() if cr else None
    return got


def check_against(got, want, states=None, crcs=None):
    """Every output equals the automaton's, byte for byte; the table's invariants hold on their own as well."""
    for k in OUTPUTS:
        if got[k] is not None:
            assert got[k].tobytes() == want[k].tobytes(), k
    n, first = len(want["extents"]), want["first"].astype(np.int64)
    assert first[0] == 0 and first[-1] == n and (np.diff(first) >= 0).all()
    assert sorted(want["patch_of"].tolist()) == list(range(n))
    assert int(want["counts"].sum()) == n
    if states is not None:
        want_s, want_c = expected_states(states, crcs, want["restarted"])
        assert (got["sha1"] == want_s).all(), "exactly the RESTARTED objects hold NewSha1()"
        assert (got["crc32"] == want_c).all()


def run_case(L, log, offsets, m, seed=0):
    states, crcs = random_states(m, np.random.default_rng(seed))
    want = automaton(log, offsets, m)
    got = twin(L, log, offsets, m, states, crcs)
    check_against(got, want, states, crcs)
    return got, want


# ---- the receiver's scripts
def test_receiver_scripts(efes_lib, golden):
    scripts = golden["patches_scripts"]["scripts"]
    assert [s["name"] for s in scripts] == ["FileReceiver", "FileReceiverNoCreate", "FileReceiverNoDelete", "FileReceiverZeroByte",
                                            "FileReceiverSingleRequest", "FileReceiverInvalidOffset"]
    # every script is one upload; interleave them round-robin into one log, as a server would see them
    records, where = [], []
    for step in range(max(len(s["patches"]) for s in scripts)):
        for i, s in enumerate(scripts):
            if step < len(s["patches"]):
                p = s["patches"][step]
                records.append((i, p["offset"], len(p["body"]), p["length"]))
                where.append((i, step))
    log = make_log(records)
    got, _ = run_case(efes_lib.lib(), log, None, len(scripts))
    for a, (i, step) in enumerate(where):
        p = scripts[i]["patches"][step]
        assert (int(got["answers"][a]["verdict"]), int(got["answers"][a]["offset"])) == (VERDICTS[p["verdict"]], p["answer"]), (scripts[i]["name"], step)
    assert got["objects"]["offset"].tolist() == [s["final_offset"] for s in scripts]
    assert got["objects"]["offset"].tolist()[:2] == [6, 3], '"foo"@0 then "bar"@3 gives 3 and 6'
    assert got["counts"].tolist() == [4, 1, 0, 2, 0]


# ---- the rules, one at a time
def test_restart_as_the_first_admitted_patch_resets_only_that_upload(efes_lib):
    log = make_log([(1, 7, 5, UNKNOWN), (0, 100, 4, UNKNOWN), (1, 0, 9, UNKNOWN), (1, 9, 2, UNKNOWN), (2, 50, 1, UNKNOWN)])
    got, want = run_case(efes_lib.lib(), log, [100, 33, 50], 3)
    assert got["answers"]["verdict"].tolist() == [EFES_PATCH_CONFLICT, EFES_PATCH_ADMITTED, EFES_PATCH_ADMITTED, EFES_PATCH_ADMITTED, EFES_PATCH_ADMITTED]
    assert got["answers"]["offset"].tolist() == [33, 104, 9, 11, 51]
    assert got["objects"]["flags"].tolist() == [0, EFES_PATCH_OBJ_RESTARTED, 0] and want["restarted"].tolist() == [False, True, False]
    assert got["objects"]["admitted"].tolist() == [1, 2, 1]


def test_restart_behind_admitted_bytes_defers_it_and_everything_behind(efes_lib):
    log = make_log([(0, 0, 3, UNKNOWN), (0, 3, 3, UNKNOWN), (0, 0, 5, UNKNOWN), (0, 6, 1, UNKNOWN), (0, 5, 1, 6), (1, 0, 2, UNKNOWN)])
    got, _ = run_case(efes_lib.lib(), log, None, 2)
    assert got["answers"]["verdict"].tolist() == [0, 0, EFES_PATCH_DEFERRED, EFES_PATCH_DEFERRED, EFES_PATCH_DEFERRED, 0]
    assert got["answers"]["offset"].tolist() == [3, 6, 6, 6, 6, 2]
    assert got["objects"]["flags"].tolist() == [EFES_PATCH_OBJ_RESTARTED | EFES_PATCH_OBJ_DEFERRED, EFES_PATCH_OBJ_RESTARTED]
    assert got["extents"]["length"].tolist() == [3, 3, 0, 0, 0, 2] and got["objects"]["offset"].tolist() == [6, 2]


def test_patches_behind_done_are_deferred(efes_lib):
    log = make_log([(0, 10, 5, 15), (0, 15, 1, UNKNOWN), (0, 0, 1, UNKNOWN), (0, 99, 1, UNKNOWN)])
    got, _ = run_case(efes_lib.lib(), log, [10], 1)
    assert got["answers"]["verdict"].tolist() == [EFES_PATCH_DONE] + [EFES_PATCH_DEFERRED] * 3
    assert got["answers"]["offset"].tolist() == [15] * 4
    assert got["objects"][0].tolist() == (15, EFES_PATCH_OBJ_DONE | EFES_PATCH_OBJ_DEFERRED, 1)
    assert got["counts"].tolist() == [0, 0, 3, 1, 0]


def test_invalid_records_land_in_the_last_segment_and_are_skipped(efes_lib):
    log = make_log([(3, 0, 4, UNKNOWN), (2, 0, 1, UNKNOWN), (0xFFFFFFFF, 0, 9, 9), (0, 0, 2, UNKNOWN), (2, 1, 1, UNKNOWN), (1 << 20, 5, 5, 5)])
    got, _ = run_case(efes_lib.lib(), log, None, 3)
    assert got["answers"]["verdict"].tolist() == [EFES_PATCH_INVALID, 0, EFES_PATCH_INVALID, 0, 0, EFES_PATCH_INVALID]
    assert got["first"].tolist() == [0, 1, 1, 6] and got["patch_of"].tolist() == [3, 0, 1, 2, 4, 5]
    assert got["answers"]["offset"].tolist() == [0, 1, 0, 2, 2, 0] and got["extents"]["length"].tolist() == [2, 0, 1, 0, 1, 0]
    assert got["objects"]["offset"].tolist() == [2, 0, 2] and got["objects"]["admitted"].tolist() == [1, 0, 2]


def test_uploads_without_a_patch_and_empty_logs(efes_lib):
    L = efes_lib.lib()
    got, _ = run_case(L, make_log([(2, 8, 1, UNKNOWN)]), [5, 6, 8, 9], 4)
    assert got["first"].tolist() == [0, 0, 0, 1, 1] and got["objects"]["offset"].tolist() == [5, 6, 9, 9]
    for m in (0, 1, 5):
        got, _ = run_case(L, make_log([]), None if m == 0 else np.arange(m) + 3, m)
        assert got["first"].tolist() == [0] * (m + 1) and got["counts"].tolist() == [0] * 5
        assert got["objects"]["offset"].tolist() == [3 + i for i in range(m)]


def test_offsets_null_is_all_zero_and_every_optional_output_may_be_null(efes_lib):
    L = efes_lib.lib()
    log = make_log([(0, 0, 3, UNKNOWN), (1, 1, 1, UNKNOWN), (1, 0, 0, 0), (0, 3, 2, 5)])
    want = automaton(log, None, 2)
    assert want["answers"]["verdict"].tolist() == [0, EFES_PATCH_CONFLICT, EFES_PATCH_DONE, EFES_PATCH_DONE]
    check_against(twin(L, log, np.zeros(2, np.uint64), 2), want)
    for k in range(1 << len(OPTIONAL)):
        drop = tuple(name for b, name in enumerate(OPTIONAL) if k >> b & 1)
        check_against(twin(L, log, None, 2, drop=drop), want)
    states, crcs = random_states(2, np.random.default_rng(3))
    assert (twin(L, log, None, 2, states=states)["sha1"] == expected_states(states, crcs, want["restarted"])[0]).all()
    assert (twin(L, log, None, 2, crcs=crcs)["crc32"] == expected_states(states, crcs, want["restarted"])[1]).all()


def test_arithmetic_wraps_at_2_to_the_64(efes_lib):
    top = MASK - 2
    log = make_log([(0, top, 5, UNKNOWN, 0), (0, 2, 1, 3, 8), (1, top, 3, 0, 16), (2, MASK, 1, UNKNOWN, 24), (2, 0, MASK, MASK, 32)])
    got, _ = run_case(efes_lib.lib(), log, [top, top, MASK], 3)
    assert got["answers"]["verdict"].tolist() == [0, EFES_PATCH_DONE, EFES_PATCH_DONE, 0, EFES_PATCH_DEFERRED]
    assert got["answers"]["offset"].tolist() == [2, 3, 0, 0, 0], "offset + length is taken modulo 2^64, as Go's int64 addition"
    assert got["extents"]["length"].tolist() == [5, 1, 3, 1, 0]


# ---- seeded random logs
def random_log(m, n, seed, objects=None):
    """The issue's mix: a uniform object per PATCH (or objects[a]); 2 % get an object index >= nobjects, 10 % an offset
    cur + 1 + r, 6 % offset 0, the rest the right offset; 10 % of the bodies are empty, the others 1..4096 bytes; half
    the uploads start at a nonzero offset; half may learn their file_length, with probability 0.15 per right-offset
    PATCH.  `cur` is what Go's sequential handling has (0 again behind a completed upload).  (log, offsets, total body
    bytes)"""
    rng = np.random.default_rng(seed)
    offsets = np.where(rng.random(m) < 0.5, rng.integers(1, 1 << 40, m), 0).astype(np.uint64)
    learns = rng.random(m) < 0.5
    cur = [int(x) for x in offsets]
    obj = rng.integers(0, m, n) if objects is None else np.asarray(objects)
    kind, empty, learn = rng.random(n), rng.random(n) < 0.10, rng.random(n) < 0.15
    lengths = np.where(empty, 0, rng.integers(1, 4097, n))
    extra = rng.integers(0, 1 << 20, n)
    beyond = rng.integers(m, 1 << 32, n)
    records, at = [], 0
    for a in range(n):
        i, ln = int(obj[a]), int(lengths[a])
        if kind[a] < 0.02:
            records.append((int(beyond[a]) if a % 3 else 0xFFFFFFFF, cur[i], ln, UNKNOWN, at))
        elif kind[a] < 0.12:
            records.append((i, cur[i] + 1 + int(extra[a]), ln, UNKNOWN, at))
        elif kind[a] < 0.18:
            records.append((i, 0, ln, UNKNOWN, at))
            cur[i] = ln
        else:
            total = cur[i] + ln if learns[i] and learn[a] else UNKNOWN
            records.append((i, cur[i], ln, total, at))
            cur[i] = 0 if total != UNKNOWN else cur[i] + ln
        at += ln
    return make_log(records), offsets, at


@pytest.fixture(scope="module")
def random_cases():
    """Per shape: the log, the offsets and the automaton's outputs, made once and left unchanged."""
    out = {}
    for m, n in RANDOM_SHAPES:
        log, offsets, _ = random_log(m, n, 1000 * m + n)
        out[(m, n)] = (log, offsets, automaton(log, offsets, m))
    return out


@pytest.mark.parametrize("m,n", RANDOM_SHAPES)
def test_random_logs_cover_every_verdict(random_cases, m, n):
    """Asserted on the oracle's output, so that no seed degenerates: every verdict covers >= 0.5 % of the PATCHes and
    ADMITTED + DONE >= 25 %."""
    for seed in (None, 0, 1):
        counts = (random_cases[(m, n)][2] if seed is None else automaton(*random_log(m, n, seed)[:2], m))["counts"].astype(np.int64)
        assert (counts * 200 >= n).all(), (seed, counts.tolist())
        assert (counts[EFES_PATCH_ADMITTED] + counts[EFES_PATCH_DONE]) * 4 >= n, (seed, counts.tolist())


@pytest.mark.parametrize("m,n", RANDOM_SHAPES)
def test_random_logs(efes_lib, random_cases, m, n):
    log, offsets, want = random_cases[(m, n)]
    states, crcs = random_states(m, np.random.default_rng(n))
    check_against(twin(efes_lib.lib(), log, offsets, m, states, crcs), want, states, crcs)


# ---- round equivalence
def sequential_replay(log, offsets, m, data):
    """Go's handling, one PATCH after the other: per PATCH (verdict, answer offset); per upload the byte strings of its
    completed files, the bytes of the unfinished one, its offset and whether its states are fresh (restarted or
    completed -- Go's deleted `.info`) or the ones it came with."""
    cur = [int(x) for x in offsets]
    files, body, fresh, answers = [[] for _ in range(m)], [b""] * m, [False] * m, []
    for p in log.tolist():
        do, ln, fo, fl, i, _ = p
        if i >= m:
            answers.append((EFES_PATCH_INVALID, 0))
            continue
        if fo == 0:
            body[i], cur[i], fresh[i] = data[do:do + ln].tobytes(), ln, True
        elif fo == cur[i]:
            body[i], cur[i] = body[i] + data[do:do + ln].tobytes(), (cur[i] + ln) & MASK
        else:
            answers.append((EFES_PATCH_CONFLICT, cur[i]))
            continue
        if cur[i] == fl:
            answers.append((EFES_PATCH_DONE, cur[i]))
            files[i].append(body[i])
            body[i], cur[i], fresh[i] = b"", 0, True
        else:
            answers.append((EFES_PATCH_ADMITTED, cur[i]))
    return answers, files, body, cur, fresh


def rounds(table, log, offsets, m, data):
    """The same through tables: `table(log, offsets)` gives the outputs of one call; the DEFERRED PATCHes are resubmitted,
    in order, until none is left.  What sequential_replay returns, and the number of rounds."""
    cur = np.array(offsets, dtype=np.uint64)
    files, body, fresh = [[] for _ in range(m)], [b""] * m, [False] * m
    answers = [None] * len(log)
    arrival = np.arange(len(log))
    nrounds = 0
    while len(log):
        nrounds += 1
        out = table(log, cur)
        ext, first = out["extents"], out["first"]
        for i in range(m):
            flags = int(out["objects"][i]["flags"])
            if flags & EFES_PATCH_OBJ_RESTARTED:
                body[i], fresh[i] = b"", True
            body[i] += b"".join(data[int(o):int(o) + int(l)].tobytes() for o, l in ext[first[i]:first[i + 1]].tolist())
            cur[i] = out["objects"][i]["offset"]
            if flags & EFES_PATCH_OBJ_DONE:  # the caller stores offset 0 and fresh states, as Go's deleted `.info` does
                files[i].append(body[i])
                body[i], cur[i], fresh[i] = b"", 0, True
        verdicts = out["answers"]["verdict"]
        for a in np.nonzero(verdicts != EFES_PATCH_DEFERRED)[0]:
            answers[arrival[a]] = (int(verdicts[a]), int(out["answers"][a]["offset"]))
        again = verdicts == EFES_PATCH_DEFERRED
        assert again.sum() < len(log), "every round decides at least one PATCH"
        log, arrival = log[again], arrival[again]
    return (answers, files, body, [int(x) for x in cur], fresh), nrounds


def check_round_equivalence(table, m, n, seed):
    log, offsets, nbytes = random_log(m, n, seed)
    data = np.random.default_rng(seed).integers(0, 256, max(nbytes, 1), dtype=np.uint8)
    want = sequential_replay(log, offsets, m, data)
    got, nrounds = rounds(table, log, offsets, m, data)
    assert nrounds > 2, "the log must need resubmitting"
    for name, g, w in zip(("answers", "completed files", "unfinished bytes", "offsets", "fresh states"), got, want):
        assert g == w, name


@pytest.mark.parametrize("m,n,seed", [(1, 40, 1), (7, 300, 2), (64, 1025, 3), (257, 2000, 4)])
def test_round_equivalence(efes_lib, m, n, seed):
    L = efes_lib.lib()
    check_round_equivalence(lambda log, offsets: twin(L, log, offsets, m), m, n, seed)


def test_standalone_sanitizer_program(tmp_path):
    """tests/cpp/patches_malformed.cpp runs the twin on heap arrays of exact size over logs of garbage, built with
    -fsanitize=address,undefined together with efes_patches.cpp and the shared rules: an out-of-range read or write
    ends it with a report.  A program of its own with the sanitizer runtimes linked in statically: it needs nothing
    preloaded and runs in the environment it is given, unchanged."""
    exe = tmp_path / "patches_malformed"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "patches_malformed.cpp"),
           os.path.join(ROOT, "efes_amd", "csrc", "efes_patches.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    missing = [line for line in built.stderr.splitlines() if "cannot find" in line and ("asan" in line or "ubsan" in line)]
    if built.returncode != 0 and missing:
        pytest.skip("the toolchain lacks the static sanitizer runtime: " + missing[0].strip())
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([str(exe)], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout[-2000:] + ran.stderr[-4000:]
    assert "logs ok" in ran.stdout
