"""The chained CRC's scan (efes_crc32_chain, efes_crc_batch.hip), restated in Python and checked against
zlib on the CPU.  A job of n bytes takes the raw register r to m (x) r ^ b (m = x^(8n), b = the raw CRC of
its bytes from zero); a head folds its in-state into b and has m = 0; validity rides along as
bad' = (a & bad) | c.  The three launches: map (per-job elements, an inclusive Hillis-Steele scan inside
each block of B jobs), carry (a scan of the block totals), finish (carry applied, tails found from the
next record).  Run with B = 8, so the carries cross many blocks, and with B = 1024.  The expectation is
a serial walk over the job list with zlib.crc32 and the validity rules of efes_hash.h spelled out."""
import random
import zlib

import pytest

from test_span_math import mulmod, raw, xpow8n

FIN, INIT, SUM_ONLY, CHAIN = 0x1, 0x2, 0x4, 0x8
ARG = -4
IDENTITY = (1 << 31, 0, 1, 0)


def compose(hi, lo):
    """hi after lo: (m2,b2,a2,c2) o (m1,b1,a1,c1)."""
    m2, b2, a2, c2 = hi
    m1, b1, a1, c1 = lo
    return (mulmod(m2, m1), mulmod(m2, b1) ^ b2, a2 & a1, (a2 & c1) | c2)


def scan_incl(elems):
    """Hillis-Steele, as the wave shuffles do it: every step reads the values of the step before."""
    cur, off = list(elems), 1
    while off < len(cur):
        cur = [compose(cur[i], cur[i - off]) if i >= off else cur[i] for i in range(len(cur))]
        off <<= 1
    return cur


def follower_bad(job, prev):
    return bool(job["sha1"] or job["state"] is None or job["state"] != prev["state"] or job["flags"] & (INIT | SUM_ONLY)
                or prev["flags"] & SUM_ONLY)


def job_map(j, jobs, states, raws):
    job = jobs[j]
    chained = bool(job["flags"] & CHAIN)
    bad = (j == 0 or follower_bad(job, jobs[j - 1])) if chained else bool(job["sha1"])
    if bad or job["state"] is None:
        return (0, 0, int(chained), int(bad))
    m, b = xpow8n(len(job["data"])), raws[j]
    if not chained:
        r_in = 0xFFFFFFFF if job["flags"] & INIT else ~states[job["state"]] & 0xFFFFFFFF
        m, b = 0, b ^ mulmod(m, r_in)
    return (m, b, int(chained), 0)


def chain_model(jobs, states, raws, B):
    """Returns (states after, per-job sum CRC or None, per-job status)."""
    n = len(jobs)
    # 1. map
    elem, btot = [], []
    for s in range(0, n, B):
        block = [job_map(j, jobs, states, raws) for j in range(s, min(s + B, n))]
        block += [IDENTITY] * (B - len(block))  # the lanes past the array
        inc = scan_incl(block)
        elem += inc[:min(B, n - s)]
        btot.append(inc[-1])
    # 2. carry
    btot = scan_incl(btot)
    # 3. finish
    out, sums, status = dict(states), [None] * n, [None] * n
    for j, job in enumerate(jobs):
        m, b, a, c = elem[j]
        if j // B:
            _, cb, _, cc = btot[j // B - 1]
            b ^= mulmod(m, cb)
            c |= a & cc
        if c:
            status[j] = ARG
            continue
        crc = ~b & 0xFFFFFFFF
        do_crc = job["state"] is not None
        tail = j + 1 == n or not jobs[j + 1]["flags"] & CHAIN or follower_bad(jobs[j + 1], job)
        if do_crc and tail and not job["flags"] & SUM_ONLY:
            out[job["state"]] = crc
        if job["flags"] & FIN:
            sums[j] = crc if do_crc else 0
        status[j] = 0
    return out, sums, status


def serial_expectation(jobs, states):
    """Write after Write with zlib, validity decided job by job."""
    out, sums, status = dict(states), [None] * len(jobs), [None] * len(jobs)
    prev_bad, cur = True, None  # cur: the CRC after the previous member of the open chain
    for j, job in enumerate(jobs):
        if job["flags"] & CHAIN:
            bad = prev_bad or j == 0 or follower_bad(job, jobs[j - 1])
        else:
            bad = bool(job["sha1"])
            if not bad and job["state"] is not None:
                cur = 0 if job["flags"] & INIT else out[job["state"]]
        prev_bad = bad
        if bad:
            status[j] = ARG
            continue
        status[j] = 0
        if job["state"] is None:
            if job["flags"] & FIN:
                sums[j] = 0
            continue
        cur = zlib.crc32(job["data"], cur)
        if job["flags"] & FIN:
            sums[j] = cur
        if not job["flags"] & SUM_ONLY:
            out[job["state"]] = cur  # the last valid member's value stays
    return out, sums, status


def seeded_jobs(rng, count=300):
    """Heads with INIT, mid-stream heads, zero-length members (in runs too), and some invalid members."""
    jobs, states, state = [], {}, -1
    for j in range(count):
        chained = j > 0 and rng.random() < 0.7
        n = 0 if rng.random() < 0.15 else rng.randrange(0, 1001)
        flags = rng.choice([0, FIN])
        if chained:
            flags |= CHAIN
        else:
            state += 1
            states[state] = rng.getrandbits(32)
            flags |= rng.choice([0, INIT])
        job = dict(data=bytes(rng.getrandbits(8) for _ in range(n)), flags=flags, state=state, sha1=False)
        roll = rng.random()
        if roll < 0.01:
            job["sha1"] = True
        elif roll < 0.02 and chained:
            job["flags"] |= rng.choice([INIT, SUM_ONLY])
        elif roll < 0.03 and chained:
            job["state"] = rng.choice([None, state - 1 if state else None])
        elif roll < 0.04 and not chained:
            job["flags"] |= SUM_ONLY
        jobs.append(job)
    return jobs, states


@pytest.fixture(scope="module")
def cases():
    out = []
    for seed in (1, 2):
        jobs, states = seeded_jobs(random.Random(seed))
        out.append((jobs, states, [raw(job["data"]) for job in jobs]))
    # CHAIN on job 0, and a chain that fills the array to its last job
    jobs = [dict(data=b"abc", flags=CHAIN | FIN, state=0, sha1=False), dict(data=b"defg", flags=INIT, state=1, sha1=False)]
    jobs += [dict(data=bytes([k]) * k, flags=CHAIN | FIN, state=1, sha1=False) for k in range(20)]
    out.append((jobs, {0: 5, 1: 6}, [raw(job["data"]) for job in jobs]))
    return out


@pytest.mark.parametrize("B", [8, 1024])
def test_three_stage_scan_matches_serial_writes(cases, B):
    for jobs, states, raws in cases:
        assert sum(1 for j in jobs if j["flags"] & CHAIN) > len(jobs) // 2
        got = chain_model(jobs, states, raws, B)
        want = serial_expectation(jobs, states)
        assert got[2] == want[2], "status"
        assert got[1] == want[1], "sums"
        assert got[0] == want[0], "states"


def test_association_order_is_free():
    """The operator is associative: a left fold, a right fold and the Hillis-Steele scan agree."""
    rng = random.Random(3)
    elems = [(rng.getrandbits(32) if rng.random() < 0.8 else 0, rng.getrandbits(32), rng.getrandbits(1), rng.getrandbits(1))
             for _ in range(37)]
    left = elems[0]
    for e in elems[1:]:
        left = compose(e, left)
    right = elems[-1]
    for e in reversed(elems[:-1]):
        right = compose(right, e)
    assert left == right == scan_incl(elems)[-1]
