"""GPU parity at compute-unit counts other than the full chip's.  Every launcher sizes its grid, its waves per
SIMD or its mode threshold by the context's CU count, which efes_ctx_create reads from the device: 256 on a whole
MI355X, and the value every other test runs with.  Here a private context's count is lowered with the test hook
efes_debug_set_cus (include/efes_testing.h) to 1, 2, 3, 8, 32 (one XCD) or the device's count - 1, which makes the
same launches a smaller device would make -- fewer workgroups, nothing else; no workgroup of these kernels waits
for another -- and drives the deepest per-workgroup code at shapes small enough for the oracle to check every job:
a workgroup of the tile pass that walks hundreds of tiles over every length edge, a wave of a chain walk that
draws ticket after ticket, the wide walk at two and three waves per SIMD with 1 650 jobs, every AUTO mode with at
most 200 jobs.

Everything is bit-exact: each case is checked per job against the oracle / hashlib / zlib through the checkers of
the files it imports its arrays from, and then byte for byte against the same call on an unhooked context
(hashing.default_context) over a second copy of the inputs (the fuzz file's run_case and the streaming digests
keep their results to themselves: there the per-job oracle check stands alone).  The grids a case relies on are asserted in the case
by restating the launcher's arithmetic over the specs.  Nothing here runs on a really partitioned device: the hook
shows that the arithmetic and the kernels are right for fewer workgroups, not that a partition's runtime behaves."""
import hashlib
import random
import zlib

import numpy as np
import pytest

import test_gpu_crc_chain as crc_chain
import test_gpu_hash_chain as hash_chain
from test_gpu_crc_batch import FIN, Jobs
from test_gpu_crc_copy import Copy, Layout
from test_gpu_fuzz import run_case
from test_gpu_hash_chain import CHAIN, INIT, OK, Chains, _seeded_states, job
from test_gpu_hash_chain_ckpt import REC, CkptChains
from test_gpu_hash_chain_group import run_mode, same_bytes
from test_gpu_hash_chain_wide import _invalid_wave, _ragged, _state_wave, run_wide
from test_gpu_parity import midstream_states, oracle_expect
from test_gpu_span import _span

pytestmark = pytest.mark.gpu

BUF_BYTES = 32 << 20  # the largest buffer the imported generators place their extents in
DST_BYTES = 40 << 20  # test_gpu_crc_copy's destination buffer
assert BUF_BYTES == crc_chain.BUF_BYTES >= hash_chain.BUF_BYTES
LAST = "device count - 1"


@pytest.fixture(scope="module")
def base(oracle):
    """What the imported helpers read from `env`, with ctx = the unhooked default context."""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import efes_amd
    from efes_amd import _lib, batch, hashing
    ctx = hashing.default_context(0)
    buf = torch.empty(BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(DST_BYTES, dtype=torch.uint8, device="cuda:0")
    assert buf.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    ctx.fill_synthetic(buf.data_ptr(), BUF_BYTES, 0x6E0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    modes = {"auto": _lib.MODE_AUTO, "wide": _lib.MODE_WIDE}
    return dict(torch=torch, efes=efes_amd, hashing=hashing, batch=batch, lib=_lib, ctx=ctx, oracle=oracle, buf=buf, dst=dst,
                host=buf.cpu().numpy(), T=_lib.EFES_CRC_BATCH_TILE, DeviceBatch=batch.DeviceBatch,
                fresh_states=batch.fresh_states, modes=modes, FIN=_lib.EFES_JOB_FINALIZE, INIT=_lib.EFES_JOB_INIT,
                device_cus=torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture
def env(request, base):
    """base with ctx = a private context whose CU count is request.param (LAST: the device's count - 1)."""
    n = base["device_cus"]
    cus = n - 1 if request.param == LAST else request.param
    if not 1 <= cus <= n:
        pytest.skip(f"the device has {n} compute units")
    small = base["hashing"].Context(0)
    try:
        small.debug_set_cus(cus)
        yield dict(base, ctx=small, cus=cus)
    finally:
        base["torch"].cuda.synchronize()
        small.close()


def at_cus(*counts):
    return pytest.mark.parametrize("env", counts, indirect=True, ids=[str(c).replace(" ", "") for c in counts])


# ---- the launchers' arithmetic, restated over the specs
def tiles_of(env, off, n, hashed=True):
    """Tiles of one job of the tile pass (efes_crc_batch.hip job_geo, tiles_of): its whole 16-byte pieces behind
    the first 16-byte boundary, 4096 to a tile; none for a job the pass does not hash."""
    head = min((16 - (env["buf"].data_ptr() + off) % 16) % 16, n)
    return ((n - head) // 16 + 4095) // 4096 if hashed else 0


def workgroup_cuts(tiles, G):
    """(q, cuts): workgroup w of G takes the tiles [w q, (w + 1) q), q = ceil(total / G); cuts = the first tiles of
    the workgroups 1.. that have any."""
    total = sum(tiles)
    q = -(-total // G)
    return q, [w * q for w in range(1, G) if w * q < total]


def tiles_behind_runs(tiles, G):
    """For every run of a job's tiles that a workgroup ends short of the job's last tile: the job's whole tiles
    behind the run, short of the last one (`after` of batch_tile_kernel, the index into tile_op[])."""
    q, _ = workgroup_cuts(tiles, G)
    out, start = [], 0
    for nt in tiles:
        for w in range(start // q, (start + nt - 1) // q + 1) if nt else ():
            a, b = max(w * q, start) - start, min((w + 1) * q, start + nt) - start
            e = min(b, nt - 1)  # the job's last tile is a run of its own
            if e > a:
                out.append(nt - 1 - e)
        start += nt
    return out


def wide_walk_waves(njobs, nchains, cus, cap=3):
    """(waves per SIMD the launcher of efes_hash_chain_wide asks for, waves per SIMD that stay on the device, the
    waves that stay in all, the tickets of 64 chains they draw): launch_hash_chain_wide_shape and the head of
    hash_chain_wide_kernel (efes_chain_wide.hip); cap = the three waves per SIMD the kernel's registers and LDS admit."""
    waves = -(-njobs // 64)
    wps = min(cap, -(-waves // (4 * cus)))
    per = 64 * 4 * wps
    grid = min(-(-njobs // per), cus)
    need = -(-nchains // 64)
    stay = min(per // 64, 4 * max(1, -(-need // (4 * grid))))
    return wps, stay // 4, grid * stay, need


# ---- 1. the hook
def test_hook_contract(base):
    """EFES_ERR_ARG outside 1 .. the device's count and for a NULL context, with nothing changed; at 2 CUs (8 SIMDs)
    every mode threshold sits at its multiple of 8; the device's count restores the device's thresholds."""
    lib, hashing, n = base["lib"], base["hashing"], base["device_cus"]
    L, G = lib.lib(), lib.MODE_GROUP
    auto = [lib.MODE_DEEP, lib.MODE_FED4, lib.MODE_FED4E, G[4], lib.MODE_WIDE]
    chain = [lib.MODE_DEEP, G[32], G[16], G[8], G[4]]

    def thresholds(ctx, cus):
        s = 4 * cus
        for fn, modes, mult in ((L.efes_auto_mode, auto, (1, 8, 12, 16)), (L.efes_hash_chain_auto_mode, chain, (1, 2, 4, 8))):
            got = [(fn(ctx.handle, m * s), fn(ctx.handle, m * s + 1)) for m in mult]
            assert got == list(zip(modes, modes[1:])), (cus, fn.__name__, got)
        assert L.efes_hash_chain_auto_mode_wide(ctx.handle, 32 * s - 1) == L.efes_hash_chain_auto_mode(ctx.handle, 32 * s - 1) != lib.MODE_WIDE
        assert L.efes_hash_chain_auto_mode_wide(ctx.handle, 32 * s) == lib.MODE_WIDE

    ctx = hashing.Context(0)
    try:
        assert L.efes_debug_set_cus(None, 1) == lib.EFES_ERR_ARG
        for bad in (0, -1, n + 1):
            assert L.efes_debug_set_cus(ctx.handle, bad) == lib.EFES_ERR_ARG, bad
            with pytest.raises(hashing.EfesError):
                ctx.debug_set_cus(bad)
        thresholds(ctx, n)  # the refused calls changed nothing
        ctx.debug_set_cus(2)
        thresholds(ctx, 2)
        assert [L.efes_auto_mode(ctx.handle, k) for k in (8, 9, 64, 65, 96, 97, 128, 129)] == \
            [auto[0], auto[1], auto[1], auto[2], auto[2], auto[3], auto[3], auto[4]]
        assert [L.efes_hash_chain_auto_mode(ctx.handle, k) for k in (8, 9, 16, 17, 32, 33, 64, 65)] == \
            [chain[0], chain[1], chain[1], chain[2], chain[2], chain[3], chain[3], chain[4]]
        assert [L.efes_hash_chain_auto_mode_wide(ctx.handle, k) for k in (255, 256)] == [chain[4], lib.MODE_WIDE]
        thresholds(base["ctx"], n)  # another context keeps the device's count
        ctx.debug_set_cus(n)
        thresholds(ctx, n)
    finally:
        ctx.close()


# ---- 2. the tile pass, efes_crc32_batch
def _boundary_specs(T):
    """The 92 jobs of test_gpu_crc_batch.test_boundaries_one_launch."""
    lengths = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, T - 1, T, T + 1, T + 64 * 7 + 5,
               2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 17, 8 * T + 13]
    rng = random.Random(21)
    specs, at = [], 0
    for n in lengths:
        for off in (0, 1, 7, 15):
            specs.append((at + off, n, rng.choice([0, 0xFFFFFFFF, rng.getrandbits(32)]), 0))
            at += (n + 16 + 4095) // 4096 * 4096
    assert at <= BUF_BYTES and len(specs) == 92
    return specs


@at_cus(1, 3, 32, LAST)
def test_tile_pass_boundaries(env, base):
    """Every length around the 16-byte piece, the tile and several tiles at four misalignments: 129 tiles, one
    per workgroup on 256 CUs, so there the pipelined walk (the next tile's bytes and job fetched under the current
    one, runs that continue, the double-buffered wave sums) never meets these edges.  One workgroup walks them all
    at cus = 1, three walk about 50 each at cus = 3, and the trailing workgroups of 32 and of the device's count - 1
    start behind the last tile.  The oracle's crc32digest per job, then the unhooked context's bytes."""
    oracle, host, cus = env["oracle"], env["host"], env["cus"]
    specs = _boundary_specs(env["T"])
    tiles = [tiles_of(env, s[0], s[1]) for s in specs]
    q, cuts = workgroup_cuts(tiles, cus)
    assert sum(tiles) == 129, "fewer tiles than a whole MI355X has workgroups"
    if cus <= 3:
        assert sum(tiles) >= 2 * cus and q >= 43
    else:
        assert len(cuts) + 1 < cus, "some workgroups start at or behind the last tile"
    A, B = Jobs(env, specs), Jobs(base, specs)
    A.batch()
    B.batch()
    crcs = A.results()[0]
    for j, (off, n, crc_in, _) in enumerate(specs):
        o = oracle.Crc32()
        o.st.crc = crc_in
        o.write(host[off:off + n].tobytes())
        assert int(crcs[j]) == o.sum32(), (cus, n, off % 4096, hex(crc_in), hex(int(crcs[j])), hex(o.sum32()))
    A.check(cus)
    same_bytes(A, B, ("boundaries", cus))


def _skew_specs(env):
    """The generator of test_gpu_crc_batch.test_skew_one_big_job_among_small (2 000 jobs of 0-300 bytes with runs of
    70, 130 or 200 jobs of 0, 3 or 15 bytes, none of which has a tile) with the 24 MiB job at the position that
    puts the second of three workgroups' first tile 130 tiles into it."""
    rng = random.Random(5)
    small = []
    while len(small) < 2000:
        if rng.random() < 0.02:
            small += [(rng.randrange(0, 1 << 20), rng.choice([0, 3, 15]), rng.getrandbits(32), 0) for _ in range(rng.choice([70, 130, 200]))]
        small.append((rng.randrange(0, 1 << 20), rng.randrange(0, 301), rng.getrandbits(32), rng.choice([0, FIN])))
    small = small[:2000]
    big = (5, (24 << 20) + 77, 0x1357, FIN)
    before = np.concatenate(([0], np.cumsum([tiles_of(env, s[0], s[1]) for s in small])))
    q = -(-(int(before[-1]) + tiles_of(env, big[0], big[1])) // 3)
    at = int(np.searchsorted(before, q - 130))
    assert before[at] == q - 130, "tiles come one at a time: some position has exactly q - 130 before it"
    return small[:at] + [big] + small[at:], at


@at_cus(1, 3, 32, LAST)
def test_tile_pass_one_big_job_among_empty_runs(env, base):
    """One 24 MiB job (385 tiles) among 2 000 small ones with runs of more than 64 consecutive jobs without a tile
    on either side: next_job's ballot loop crosses them inside a workgroup's walk.  At cus = 3 a workgroup's range
    ends 130 tiles into the big job, so that run is advanced over the 254 tiles behind it (tile_op[254]); at the
    device's count - 1 the runs are a few tiles long and the first ones have more than 256 tiles behind them
    (tile_op[after % 256] and the square-and-multiply factor).  zlib per job, then the unhooked context's bytes."""
    cus = env["cus"]
    specs, at = _skew_specs(env)
    tiles = [tiles_of(env, s[0], s[1]) for s in specs]
    assert tiles[at] == 385
    empty = "".join("1" if t else "0" for t in tiles)
    assert "0" * 65 in empty[:at] and "0" * 65 in empty[at + 1:], "runs of more than 64 jobs without a tile"
    behind = tiles_behind_runs(tiles, cus)
    if cus <= 3:
        assert sum(tiles) >= 2 * cus
    if cus == 1:
        assert not any(behind), "one workgroup: every run ends at its job's last whole tile"
    if cus == 3:
        assert max(behind) == 254
    if cus >= 128:
        assert max(behind) > 256 and any(a % 256 for a in behind if a > 256)
    A, B = Jobs(env, specs), Jobs(base, specs)
    A.batch()
    B.batch()
    A.check(cus)
    same_bytes(A, B, ("skew", cus))


# ---- 3. the tile pass, efes_crc32_chain and efes_crc32_copy
CHAIN_SEED = 3


def _crc_chains(env, cus):
    """40 seeded chains of 1-8 extents of up to 1 MiB (test_gpu_crc_chain._seeded_chains), and their tiles."""
    jobs, crc_in = crc_chain._seeded_chains(random.Random(CHAIN_SEED), 40)
    tiles = [tiles_of(env, s["off"], s["n"], s["state"] is not None and not s["sha1"]) for s in jobs]
    assert sum(tiles) >= 2 * cus
    if cus == 3:  # both cuts fall inside a chain: the tiles on either side of them are the same object's
        owner = np.repeat([s["state"] for s in jobs], tiles)
        q, cuts = workgroup_cuts(tiles, cus)
        assert len(cuts) == 2 and all(owner[c - 1] == owner[c] for c in cuts), (q, cuts)
        starts = set(np.cumsum(tiles).tolist())
        assert any(c not in starts for c in cuts), "a cut inside an extent"
    return jobs, crc_in


@at_cus(1, 3)
def test_tile_pass_chains(env, base):
    """Chained CRC jobs whose objects straddle the workgroups' ranges: zlib of each object's concatenation, the
    running sums, then the unhooked context's bytes."""
    jobs, crc_in = _crc_chains(env, env["cus"])
    A, B = crc_chain.Chains(env, jobs, crc_in), crc_chain.Chains(base, jobs, crc_in)
    A.run()
    B.run()
    assert (A.check(env["cus"]) == 0).all()
    same_bytes(A, B, ("crc chain", env["cus"]))


@at_cus(1, 3)
def test_tile_pass_copy(env, base):
    """The same chains through efes_crc32_copy: destinations at 0, 1 and 8 mod 16 in turn, every fifth NULL.  The
    copy file's checker (the whole destination image with its guard bytes, efes_crc32_chain's bytes, zlib over what
    landed), then the unhooked context's image and bytes."""
    jobs, crc_in = _crc_chains(env, env["cus"])
    lay, dsts = Layout(), []
    for j, s in enumerate(jobs):
        d = lay.place(s["n"], [0, 1, 8][j % 3])
        dsts.append(None if j % 5 == 4 else d)
    assert {d % 16 for d in dsts if d is not None} == {0, 1, 8}
    A = Copy(env, jobs, crc_in, dsts)
    A.run()
    status, img = A.check(env["cus"])
    assert (status == 0).all()
    img = img.copy()
    B = Copy(base, jobs, crc_in, dsts)
    B.run()
    _, ref = B.check("unhooked")
    assert img.tobytes() == ref.tobytes()
    same_bytes(A.copy, B.copy, ("crc copy", env["cus"]))


# ---- 4. the span
@at_cus(1, 3)
def test_span_rows_per_workgroup(env, base):
    """k * 65536 + d bytes, k = 1..13, d in {0, 64 * 7 + 5}, at offsets 0 and 7 from random in-states: up to 13 rows
    of 1024 lines on one to three workgroups, so a workgroup takes several rows, the rows divide unevenly, and the
    partial row falls to each owner.  zlib, then the unhooked context's value."""
    host = env["host"]
    rng = random.Random(13)
    for k in range(1, 14):
        for d in (0, 64 * 7 + 5):
            for off in (0, 7):
                n, crc_in = k * 65536 + d, rng.getrandbits(32)
                got = _span(env, env["buf"], off, n, crc_in)
                assert got == zlib.crc32(host[off:off + n], crc_in), (env["cus"], k, d, off, hex(crc_in))
                assert got == _span(base, base["buf"], off, n, crc_in)


# ---- 5. the chain walks
ENTRIES = ["chain", "group4", "group8", "group16", "group32", "ckpt-deep", "ckpt-group4", "wide", "wide-ckpt"]


def _walk(env, entry, specs, states_in, crc_in):
    """One copy of the inputs through one entry point on env's context."""
    lib = env["lib"]
    C = (CkptChains if "ckpt" in entry else Chains)(env, specs, states_in, crc_in)
    if entry == "chain":
        C.run()
    elif entry.startswith("group"):
        run_mode(C, lib.MODE_GROUP[int(entry[5:])])
    elif entry == "ckpt-deep":
        C.run_ckpt(lib.MODE_DEEP)
    elif entry == "ckpt-group4":
        C.run_ckpt(lib.MODE_GROUP[4])
    else:
        run_wide(C, ckpt=C.ptrs.data_ptr() if entry == "wide-ckpt" else None)
    return C


@pytest.mark.parametrize("entry", ENTRIES)
@at_cus(1, 3)
def test_chain_walks(env, base, entry):
    """129 ragged chains (1-9 members of 0-700 bytes), the wave of every invalidity rule and the wave of Go's panic
    states through efes_hash_chain, efes_hash_chain_mode at every G, efes_hash_chain_checkpoints (the wave walk and
    G = 4) and efes_hash_chain_wide without and with records.  On 256 CUs a wave draws a second chain only beyond
    1 024 chains; on one CU 129 chains make every wave of the wave walk and of the grouped walks draw ticket after
    ticket, with the chain's state, its bad flag and its record pointer reset between the draws, and a wave that has
    met an invalid or panicking chain goes on to clean ones.  (The wide walk draws 64 chains at a time and sizes its
    waves by the chain count: its second draws are test_wide_walk_waves_per_simd's last case; here its workgroup of
    one CU holds the waves of three.)  The oracle per job, the records, then
    the unhooked context's bytes."""
    cus = env["cus"]
    arrays = [("ragged",) + _ragged(env, random.Random(129), 129),
              ("invalid", _invalid_wave()[0]) + _seeded_states(env, random.Random(500), 65),
              ("panic",) + _state_wave(env)[:3]]
    for what, specs, states_in, crc_in in arrays:
        A, B = _walk(env, entry, specs, states_in, crc_in), _walk(base, entry, specs, states_in, crc_in)
        A.check((what, entry, cus))
        same_bytes(A, B, (what, entry, cus))
        if "ckpt" in entry:
            A.check_records((what, entry, cus))
            assert A.records().tobytes() == B.records().tobytes(), (what, entry, cus)


# ---- 6. the wide walk's waves per SIMD
@pytest.mark.parametrize("env,chains,members,want", [(2, 300, (2, 2), (2, 1)), (2, 600, (1, 2), (2, 2)), (2, 1100, (1, 2), (3, 3)),
                                                     (1, 900, (1, 2), (3, 3))], indirect=["env"],
                         ids=["2-300x2-second-waves-leave", "2-600-two-waves", "2-1100-three-waves", "1-900-second-draws"])
def test_wide_walk_waves_per_simd(env, base, chains, members, want):
    """On 2 CUs (8 SIMDs): 600 jobs make the launcher ask for 2 waves per SIMD while their 300 chains fill less than
    one, so the second waves leave behind the barrier; 600 chains keep 2; 1 100 chains of about 1 650 jobs run at 3
    (66 000 and 140 000 chains on 256 CUs).  On one CU 900 chains are 15 tickets for the 12 waves that three per SIMD
    are, so some wave draws a second 64 chains (more than 196 608 chains on 256 CUs), its lanes' states, bad flags
    and x buffers set up again.  Members of 0-130 bytes, fused, SHA-1-only and CRC-only chains, FINALIZE at random.
    The oracle on every job and every record, records and bytes against efes_hash_chain_checkpoints(EFES_MODE_GROUP4),
    the record-less call, then the unhooked context's bytes."""
    lib = env["lib"]
    rng = np.random.default_rng(chains)
    count = rng.integers(members[0], members[1] + 1, size=chains)
    n = int(count.sum())
    owner = np.repeat(np.arange(chains), count)
    head = np.concatenate(([True], owner[1:] != owner[:-1]))
    lens = rng.integers(0, 131, size=n)
    offs = rng.integers(0, hash_chain.BUF_BYTES - 130, size=n)
    kind = owner % 3  # fused, SHA-1-only, CRC-only
    flags = np.where(head, INIT, CHAIN) | np.where(rng.integers(0, 2, size=n) == 1, hash_chain.FIN, 0)
    specs = [job(int(offs[j]), int(lens[j]), int(flags[j]), int(owner[j]) if kind[j] != 2 else None,
                 int(owner[j]) if kind[j] != 1 else None) for j in range(n)]
    wps, stay, waves, tickets = wide_walk_waves(n, chains, env["cus"])
    assert (wps, stay) == want and (tickets > waves) == (chains == 900), (n, chains, wps, stay, waves, tickets)
    if members == (1, 2):
        assert 1.4 * chains < n < 1.6 * chains
    fresh, crc_in = np.zeros(chains, dtype=lib.SHA1_STATE_DTYPE), np.zeros(chains, np.uint32)
    W, D = CkptChains(env, specs, fresh, crc_in, stride=REC), CkptChains(env, specs, fresh, crc_in, stride=REC)
    N, U = Chains(env, specs, fresh, crc_in), CkptChains(base, specs, fresh, crc_in, stride=REC)
    run_wide(W, ckpt=W.ptrs.data_ptr())
    D.run_ckpt(lib.MODE_GROUP[4])
    run_wide(N)
    run_wide(U, ckpt=U.ptrs.data_ptr())
    _, _, _, estatus = W.check(chains)
    assert (estatus == OK).all()
    due, _ = W.check_records(chains)
    assert due.all()
    for other, what in ((D, "EFES_MODE_GROUP4"), (N, "no records"), (U, "unhooked")):
        same_bytes(W, other, (chains, what))
    assert W.records().tobytes() == D.records().tobytes() == U.records().tobytes()


# ---- 7. the submit path
@pytest.mark.parametrize("n", [8, 40, 90, 120, 200])
@at_cus(2)
def test_submit_auto_resolves_to_every_shape(env, oracle, n):
    """efes_hash_submit (EFES_MODE_AUTO) on 2 CUs: 8, 40, 90, 120 and 200 jobs resolve to DEEP, FED4, FED4E, GROUP4
    and WIDE (from 1 025 / 8 193 / 12 289 / 16 385 jobs on 256 CUs).  The fuzz file's random batch and its per-job
    oracle check."""
    lib = env["lib"]
    shape = {8: lib.MODE_DEEP, 40: lib.MODE_FED4, 90: lib.MODE_FED4E, 120: lib.MODE_GROUP[4], 200: lib.MODE_WIDE}
    assert lib.lib().efes_auto_mode(env["ctx"].handle, n) == shape[n]
    run_case(env, oracle, 7000 + n, "auto", n)


@at_cus(2)
def test_submit_wide_three_waves_per_simd(env, oracle):
    """EFES_MODE_WIDE with 1 300 jobs on 2 CUs: launch_wide's three waves per SIMD (more than 131 072 jobs on 256
    CUs) in two workgroups of 12 waves, paced by wide_pace."""
    n, cus = 1300, env["cus"]
    waves = -(-n // 64)
    wps = min(3, -(-waves // (4 * cus)))  # launch_wide (efes_kernels.hip)
    assert wps == 3 and -(-n // (64 * 4 * wps)) == 2
    run_case(env, oracle, 1300, "wide", n)


@at_cus(8, 32)
def test_planned_batch(env, base):
    """efes_plan_batch with a capacity of 8 and of 32 CUs over 200 jobs of test_planned_batch_random_lengths' mix
    (log-normal, capped at 6 MiB, some empty): the order is a permutation, longest first, the 1..4 parts sum to
    the job count, and the planned launch gives the oracle's digests and the unhooked context's bytes."""
    from efes_amd.batch import MODE_PLAN
    oracle, torch = env["oracle"], env["torch"]
    rng = np.random.default_rng(31 + env["cus"])
    n = 200
    lengths = np.minimum(rng.lognormal(10.0, 2.0, n).astype(np.int64), 6 << 20)
    lengths[rng.integers(0, n, 5)] = 0
    offsets = np.concatenate([[0], np.cumsum(lengths + 17)[:-1]]).astype(np.uint64)
    host = oracle.fill_synthetic(int((lengths + 17).sum()) + 64, 2024)
    buf = torch.from_numpy(host).to("cuda:0")
    order, plan = env["ctx"].plan(lengths)
    assert sorted(order.tolist()) == list(range(n)) and (np.diff(lengths[order]) <= 0).all()
    assert 1 <= plan.nparts <= 4 and plan.njobs == n and sum(p[0] for p in plan.parts()) == n
    b = env["DeviceBatch"](buf.data_ptr(), offsets, lengths, fresh=True, ctx=env["ctx"])
    u = env["DeviceBatch"](buf.data_ptr(), offsets, lengths, fresh=True, ctx=base["ctx"])
    b.make_plan()
    assert b.plan.parts() == plan.parts()
    b.run(MODE_PLAN)
    u.run(MODE_PLAN)
    assert (b.status_host() == 0).all()
    got = list(zip(b.sha1_hex(), b.crc_sum().tolist()))
    for i in range(n):
        assert got[i] == oracle.hash_message(host[int(offsets[i]):int(offsets[i]) + int(lengths[i])]), (i, int(lengths[i]))
    for f in ("states_host", "crc_sum", "sums_host", "status_host"):
        assert getattr(b, f)().tobytes() == getattr(u, f)().tobytes(), f


# ---- 8. the shapes of jobs read over PCIe
@pytest.mark.parametrize("n", [4, 8, 16, 32, 40])
@at_cus(1)
def test_host_jobs_read_in_place(env, base, oracle, n):
    """efes_hash_host over pinned host memory read in place: with 4 SIMDs, 4, 8, 16, 32 and 40 jobs take pcie_mode's
    DEEP, GROUP32, GROUP16, GROUP8 and GROUP4 (the ladder of efes_hash_chain_auto_mode, asserted through it; from
    1 025 jobs on 256 CUs).  Mid-stream in-states; the oracle per job, then the unhooked context's bytes."""
    from efes_amd._lib import EFES_HOST_ZERO_COPY
    from efes_amd.batch import HostBatch, PinnedHostBuffer
    lib = env["lib"]
    ladder = {4: lib.MODE_DEEP, 8: lib.MODE_GROUP[32], 16: lib.MODE_GROUP[16], 32: lib.MODE_GROUP[8], 40: lib.MODE_GROUP[4]}
    assert env["hashing"].hash_chain_auto_mode(n, env["ctx"]) == ladder[n]
    rng = random.Random(800 + n)
    lengths = [rng.choice([0, 1, 64, 65, 4095, 100000] + [rng.randint(0, 150000)] * 6) for _ in range(n)]
    offsets, pos = [], 0
    for length in lengths:
        offsets.append(pos)
        pos += length + rng.randint(0, 7)
    buf = PinnedHostBuffer(pos + 8, env["ctx"])
    try:
        buf.array[:] = oracle.fill_synthetic(pos + 8, 6 + n)
        states, crcs = midstream_states(oracle, env, n, random.Random(n))
        hb = HostBatch(buf.ptr, offsets, lengths, fresh=False, states=states, crcs=crcs, ctx=env["ctx"])
        ub = HostBatch(buf.ptr, offsets, lengths, fresh=False, states=states, crcs=crcs, ctx=base["ctx"])
        st = hb.run(EFES_HOST_ZERO_COPY)
        ub.run(EFES_HOST_ZERO_COPY)
        assert st.segments == 1 and st.bytes == sum(lengths)
        for i, (o, length) in enumerate(zip(offsets, lengths)):
            d = buf.array[o:o + length].tobytes()
            e_status, e_state, e_crc, e_sum = oracle_expect(oracle, states[i], d, int(crcs[i]))
            assert hb.status[i] == e_status == 0, (n, i)
            assert list(hb.states[i]["h"]) == e_state["h"] and bytes(hb.states[i]["x"]) == e_state["x"], (n, i)
            assert int(hb.states[i]["nx"]) == e_state["nx"] and int(hb.states[i]["len"]) == e_state["len"], (n, i)
            assert int(hb.crcs[i]) == e_crc and bytes(hb.sums[i]) == e_sum + e_crc.to_bytes(4, "big"), (n, i)
        for f in ("states", "crcs", "sums", "status"):
            assert getattr(hb, f).tobytes() == getattr(ub, f).tobytes(), (n, f)
    finally:
        buf.free()


@at_cus(1)
def test_digest_queue_batches_beyond_one_job_per_simd(env):
    """40 CRC + SHA-1 digest pairs on the hooked context, every Write made before the first Sum, so the digest
    queue's launches may hold more chunks than the 4 SIMDs it sizes its shape by.  hashlib and zlib."""
    h = env["hashing"]
    rng = random.Random(40)
    datas = [[rng.randbytes(rng.choice([0, 1, 63, 64, 65, 4096, rng.randrange(0, 70000)])) for _ in range(rng.randrange(1, 4))]
             for _ in range(40)]
    pairs = []
    try:
        for _ in datas:
            pairs.append((h.CRC32Digest(env["ctx"]), h.Sha1Digest(env["ctx"])))
        for step in range(3):
            for (c, s), parts in zip(pairs, datas):
                if step < len(parts):  # filereceiver.go:208 io.MultiWriter(f, CRC32, Sha1): CRC first
                    c.write(parts[step])
                    s.write(parts[step])
        for i, ((c, s), parts) in enumerate(zip(pairs, datas)):
            whole = b"".join(parts)
            assert s.sum().hex() == hashlib.sha1(whole).hexdigest(), i
            assert c.sum32() == zlib.crc32(whole), i
    finally:  # the digests go before their context does
        for c, s in pairs:
            c.__del__()
            s.__del__()


# ---- 9. DeviceObjects
@pytest.mark.parametrize("walk", ["auto", "auto_wide"])
@at_cus(1)
def test_device_objects_walk(env, base, walk, monkeypatch):
    """3, 7, 14, 30, 60 and 130 objects of 1-9 extents on one CU: walk="auto" takes efes_hash_chain_auto_mode's
    EFES_MODE_DEEP, GROUP32, GROUP16, GROUP8 and GROUP4, and walk="auto_wide" calls the wide walk at 130 (from 32 768
    objects on 256 CUs).  hashlib and zlib per object, then everything walk=None gives on the unhooked context."""
    batch, lib, hashing, host = env["batch"], env["lib"], env["hashing"], env["host"]
    G = lib.MODE_GROUP
    want = {3: lib.MODE_DEEP, 7: G[32], 14: G[16], 30: G[8], 60: G[4], 130: lib.MODE_WIDE if walk == "auto_wide" else G[4]}
    calls = []
    orig = type(env["ctx"]).hash_chain_wide
    monkeypatch.setattr(type(env["ctx"]), "hash_chain_wide", lambda self, *a: calls.append(self) or orig(self, *a))
    rng = random.Random(1300)
    for count in want:
        objects = [[(rng.randrange(0, hash_chain.BUF_BYTES - 3000), rng.choice([0, rng.randrange(0, 3000)])) for _ in range(1 + k % 9)]
                   for k in range(count)]
        O = batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, running=True, walk=walk, ctx=env["ctx"])
        P = batch.DeviceObjects(env["buf"].data_ptr(), objects, sha1=True, running=True, ctx=base["ctx"])
        auto = hashing.hash_chain_auto_mode_wide if walk == "auto_wide" else hashing.hash_chain_auto_mode
        assert O.walk == auto(count, env["ctx"]) == want[count], count
        del calls[:]
        O.run()
        P.run()
        assert calls == ([env["ctx"]] if want[count] == lib.MODE_WIDE else []), count
        assert (O.status_host() == OK).all()
        whole = [b"".join(bytes(host[a:a + m]) for a, m in o) for o in objects]
        assert O.sha1_hex() == [hashlib.sha1(w).hexdigest() for w in whole], count
        assert O.crc_sum().tolist() == [zlib.crc32(w) for w in whole], count
        assert O.status_host().tobytes() == P.status_host().tobytes()
        assert O.states_host().tobytes() == P.states_host().tobytes()
        assert O.crc_sum().tobytes() == P.crc_sum().tobytes()
        assert O.running_sha1() == P.running_sha1() and O.running_crcs().tobytes() == P.running_crcs().tobytes()
