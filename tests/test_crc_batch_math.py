"""The batched CRC's decomposition (efes_crc_batch.hip), restated in Python and checked against zlib
on the CPU: every job's whole 16-byte pieces cut into tiles, the tiles of all jobs dealt to G
workgroups in consecutive ranges, each lane folding its pieces with the two stride operators (inside a
tile, into the next tile) over a run of tiles of one job, advanced at the end of the run over the
pieces behind its last one and the job's tiles behind the run, the job's last tile kept apart in a
second accumulator, and the finish formula.  Small tiles so every case runs in milliseconds; the GPU
tests (tests/test_gpu_crc_batch.py) check the kernels."""
import random
import zlib

from test_span_math import mulmod, raw, xpow8n

PIECE = 16


def batch_model(jobs, lanes: int, per_lane: int, G: int):
    """jobs: [(buf, head, crc_in)] with head < 16 the bytes before the first piece; returns the CRCs."""
    P = lanes * per_lane  # pieces per tile
    T = P * PIECE
    lane_stride, tile_stride = xpow8n(PIECE * lanes), xpow8n(T - (per_lane - 1) * PIECE * lanes)
    geo = []
    for buf, head, _ in jobs:
        head = min(head, len(buf))
        m = len(buf) - head
        geo.append((head, m // PIECE, m % PIECE))
    ntile = [(np_ + P - 1) // P for _, np_, _ in geo]
    tiles = [(j, i) for j in range(len(jobs)) for i in range(ntile[j])]  # the prefix sum, spelled out
    acc_main, acc_last = [0] * len(jobs), [0] * len(jobs)
    q = (len(tiles) + G - 1) // G
    for w in range(G):
        mine = tiles[w * q:(w + 1) * q]
        acc = [0] * lanes
        for n, (j, i) in enumerate(mine):
            buf, _, _ = jobs[j]
            head, np_, _ = geo[j]
            kv = [0] * lanes
            for lane in range(lanes):
                for k in range(per_lane):
                    p = i * P + k * lanes + lane
                    if p < np_:
                        r = raw(buf[head + p * PIECE:head + (p + 1) * PIECE])
                        acc[lane] = mulmod(tile_stride if k == 0 else lane_stride, acc[lane]) ^ r
                        kv[lane] = k + 1
            last = i + 1 == ntile[j]
            nxt = mine[n + 1] if n + 1 < len(mine) else None
            cont = not last and nxt is not None and nxt[0] == j and nxt[1] + 1 != ntile[j]
            if cont:
                continue
            in_tile = min(P, np_ - i * P)
            x = 0
            for lane in range(lanes):
                if kv[lane]:
                    x ^= mulmod(xpow8n(PIECE * (in_tile - 1 - (lane + lanes * (kv[lane] - 1)))), acc[lane])
                acc[lane] = 0
            if last:
                acc_last[j] ^= x
            else:
                acc_main[j] ^= mulmod(xpow8n(T * (ntile[j] - 2 - i)), x)
    out = []
    for j, (buf, _, crc_in) in enumerate(jobs):
        head, np_, rest = geo[j]
        r = ~zlib.crc32(buf[:head], crc_in) & 0xFFFFFFFF  # the register after the head bytes
        bulk = 0
        if np_:
            last_bytes = PIECE * np_ - (ntile[j] - 1) * T
            bulk = mulmod(xpow8n(last_bytes), acc_main[j]) ^ acc_last[j]
        tail = raw(buf[head + np_ * PIECE:])
        total = mulmod(xpow8n(len(buf) - head), r) ^ mulmod(xpow8n(rest), bulk) ^ tail
        out.append(~total & 0xFFFFFFFF)
    return out


def test_batch_decomposition_matches_zlib():
    rng = random.Random(8)
    for lanes, per_lane, G in [(1, 1, 1), (2, 2, 1), (4, 4, 3), (3, 2, 5), (8, 4, 4), (4, 3, 7)]:
        T = lanes * per_lane * PIECE
        for _ in range(3):
            jobs = []
            for _ in range(rng.randrange(1, 9)):
                n = rng.choice([0, rng.randrange(0, 40), rng.randrange(0, 3 * T), rng.randrange(0, 9 * T), 2 * T, T + 15])
                jobs.append((bytes(rng.getrandbits(8) for _ in range(n)), rng.randrange(16), rng.getrandbits(32)))
            got = batch_model(jobs, lanes, per_lane, G)
            assert got == [zlib.crc32(b, c) for b, _, c in jobs], (lanes, per_lane, G, [len(b) for b, _, _ in jobs])
