// efes_crc_batch.hip -- CRC-32/IEEE of MANY device buffers in one call, each spread over the whole GPU
// (efes_crc32_batch, ABI 8), of objects that lie in many extents (efes_crc32_chain, further down), and
// the same with the bytes copied to a destination per job in the pass that hashes them (efes_crc32_copy).
//
// CRC-only jobs of efes_hash_submit run in the SHA-1-shaped kernels, one wavefront per job at best,
// although CRC-32 is GF(2)-linear and needs no chain (efes_crc_span.hip has the identities).  Here
// the jobs' bytes are cut into tiles of T = EFES_CRC_BATCH_TILE bytes and the tiles, not the jobs,
// are dealt to the workgroups.  The lengths live on the device, so the decomposition is done there,
// in three stream-ordered launches over the caller's scratch:
//   * batch_prep_kernel (one lane per job): a job's bulk is the np = (length - head) / 16 whole
//     16-byte pieces behind its first 16-byte boundary; tiles(job) = ceil(np / 4096), 0 for a job
//     that carries a SHA-1 state or no CRC state.  Writes the exclusive prefix sum of tiles() within
//     each block of 1024 jobs (loc[]), the block's sum (bsum[]), and zeroes the job's two 4-byte
//     accumulators.  Counts are 64-bit.
//   * batch_tile_kernel (the hot path; one workgroup of 1024 lanes per CU): every workgroup scans
//     bsum[] (<= 1024 entries) into LDS, which gives the tile total; workgroup w takes the
//     consecutive tiles [w q, (w+1) q), q = ceil(total / G).  It finds its first tile's job by two
//     counting passes (blocks, then the jobs of one block) and walks on from there: the next job with
//     tiles is found by one coalesced read of 64 prefix entries per wave and a ballot, fetched while
//     the current tile is hashed, as are the next tile's bytes.  Lane j of wave v reads the pieces
//     256 v + 64 k + j (k = 0..3: four coalesced 1 KiB wave reads), takes each piece's raw CRC by
//     slicing-by-4 from lane-private table copies in LDS (the layout of span_kernel) and folds
//     acc = Z^stride(acc) ^ raw with two fixed byte-sliced operator tables (1024 bytes between a
//     lane's pieces in a tile, T - 3072 to its first piece of the next tile).  A run of tiles of one
//     job is folded this way without leaving the registers; at the end of a run each lane is
//     advanced over the pieces that follow its last one (piece_op[]), the workgroup is XOR-reduced,
//     advanced over the job's tiles behind the run (tile_op[], square-and-multiply beyond 256) and
//     XORed into the job's accumulator with one atomic.  A job's LAST tile (whole or partial) is a
//     run of its own and goes to the second accumulator, because what is still to be applied to it
//     differs: acc_main waits for Z^(bytes of the last tile), acc_last for nothing.
//   * batch_finish_kernel (one lane per job): head (< 16) and rest (< 16) bytes byte-wise
//     (crc32.go:125), crc' = ~(Z^m(~crc_head) ^ Z^rest(Z^Lb(acc_main) ^ acc_last) ^ raw(rest)), and
//     the state, sum and status stores exactly as the job kernels make them (efes_kernels.hip
//     deep_rest) for a job without SHA-1; a job with a SHA-1 state gets EFES_ERR_ARG and nothing else.
// No workgroup waits for another: stream order between the launches is the only dependency, and
// every loop bound comes from memory the previous launch wrote.  Atomics go to the scratch only.
// Plain HIP: no inline assembly, no LDS-DMA.
//
// Bound: HBM read, every byte once, plus per tile one 512-byte prefix read per wave, and per run one
// gf2 product per lane and two or three on one lane.  Measured rates per shape, against the job
// kernels and the span: DESIGN.md §4 "Batched CRC" (profiles/crc_batch/bench.json).
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   batch_prep_kernel     60 VGPRs, 22 SGPRs,    128 B LDS, no scratch, no spills, 8 waves/SIMD
//   batch_tile_kernel    107 VGPRs, 97 SGPRs, 82 432 B LDS, no scratch, no spills, 4 waves/SIMD (one
//                        1024-lane workgroup per CU; half of the CU's 160 KiB LDS)
//   batch_finish_kernel   75 VGPRs, 29 SGPRs,      0 B LDS, no scratch, no spills, 6 waves/SIMD
//
// Chained jobs (efes_crc32_chain): a job with EFES_JOB_CHAIN is the next Write into the state of the
// job before it, so one object may lie in many extents.  The prep and tile kernels run unchanged (an
// extent is dealt to the workgroups as the same extent would be as a job of its own); the finish pass
// is replaced by a scan.  A job of n bytes takes the raw register r to m (x) r ^ b with m = x^(8n) and
// b = the raw CRC of its bytes from a zero register; a head folds its in-state into b and has m = 0,
// so it drops whatever stands before it and chains need no segment flags.  Validity rides along as
// bad' = (a & bad) | c (a: the job is chained, c: it is invalid by itself).  Maps compose as
// (m2,b2,a2,c2) o (m1,b1,a1,c1) = (m2 (x) m1, m2 (x) b1 ^ b2, a2 & a1, (a2 & c1) | c2), so the register
// and the bad bit after every job are an inclusive scan, in three stream-ordered launches over
// 16-byte elements behind the batch scratch:
//   * chain_map_kernel (one lane per job, 1024 jobs per workgroup): builds the job's map from its
//     head and rest bytes and the two accumulators (as batch_finish_kernel combines them), reads the
//     in-state of a head, scans the workgroup (wave shuffles, then the 16 wave totals through LDS) and
//     stores elem[job] and the block's total.  States are read here and written only by
//     chain_finish_kernel, so the two never race.
//   * chain_carry_kernel (one workgroup, one lane per block, whole waves): scans the <= 1024 block totals
//     in place.  Skipped for one block.
//   * chain_finish_kernel (one lane per job): applies the carry of the blocks before; an invalid job
//     gets EFES_ERR_ARG and nothing else; a valid one its sum under FINALIZE and its status, and the
//     tail of a chain (the last job, or one whose successor is unflagged or invalid by itself) stores
//     the state.
// No workgroup waits for another here either.
//   chain_map_kernel      68 VGPRs, 43 SGPRs,    256 B LDS, no scratch, no spills, 7 waves/SIMD
//   chain_carry_kernel    68 VGPRs, 39 SGPRs,    256 B LDS, no scratch, no spills, 7 waves/SIMD
//   chain_finish_kernel   50 VGPRs, 20 SGPRs,      0 B LDS, no scratch, no spills, 8 waves/SIMD
//
// Copy with CRC (efes_crc32_copy): efes_crc32_chain with two of its five launches replaced by copying
// instantiations of the same code; prep, carry and finish are reused, and so is the scratch layout.
//   * batch_tile_kernel<true>: the tile pass holds every 16-byte piece of every job in registers, so it
//     stores each piece it hashes to dst[job] + head + 16 piece, under the predicate that guards the
//     piece's load (zero-padded pieces are never stored).  The source side is 16-byte aligned by
//     construction (job_geo); the destination of a piece is not, so the store goes through a pointer
//     of alignment 1: still one global_store_dwordx4, and a wave still writes 1 KiB contiguously.
//     Plain stores; relative misalignment costs under 2 % (DESIGN.md §4 "Copy with CRC").
//     dst[job] == NULL: no store.
//     batch_tile_kernel<false> is the pass of the other two calls: its code differs from the
//     untemplated kernel's in the order of two scalar moves.
//   * copy_map_kernel: chain_map_kernel whose lane also lands the job's head and rest bytes, which it
//     reads byte by byte anyway.  It skips what chain_map_kernel skips: a job with sha1 != NULL or
//     crc32 == NULL, which has no tiles either, is not copied at all; a member that is invalid by its
//     flags or its state pointer has its pieces copied (validity is known only after the scan) but not
//     its head and rest.
//   batch_tile_kernel<true>  107 VGPRs, 103 SGPRs, 82 432 B LDS, no scratch, no spills, 4 waves/SIMD
//   copy_map_kernel           68 VGPRs,  43 SGPRs,    256 B LDS, no scratch, no spills, 7 waves/SIMD
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "efes_gf2.hpp"
#include "efes_internal.hpp"

namespace efes {

namespace {

constexpr uint64_t kTile = EFES_CRC_BATCH_TILE;
constexpr int kPerLane = kBatchPieces / kBatchLanes;  // pieces of one tile per lane
constexpr int kWaves = kBatchLanes / 64;
constexpr uint32_t kPrefixBlock = 1024;  // jobs per block of the prefix sum
constexpr uint32_t kMaxBlocks = EFES_CRC_BATCH_MAX_JOBS / kPrefixBlock;
constexpr uint64_t kLaneStride = 16 * 64;  // bytes between a lane's pieces k and k + 1 (one 1 KiB wave read)
constexpr uint64_t kTileStride = kTile - (kPerLane - 1) * kLaneStride;  // from piece kPerLane-1 to piece 0 of the next tile
static_assert(kTile == 65536 && kPerLane == 4 && kLaneStride == 1024, "the piece layout below");
static_assert(kMaxBlocks <= kBatchLanes, "one lane per block sum");
static_assert(kTile * kBatchTileOps == (1ull << 24), "tile_op covers 2^24 bytes (batch_flush)");

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef v4u v4u_u __attribute__((aligned(1)));  // a piece at its destination (efes_crc32_copy): any alignment

// Scratch: bsum[kMaxBlocks] | loc[njobs] | acc[njobs] (main, last).
struct Scratch {
  uint64_t* bsum;
  uint64_t* loc;
  uint2* acc;
};
__host__ __device__ inline Scratch scratch_of(void* p, uint32_t njobs) {
  Scratch s;
  s.bsum = static_cast<uint64_t*>(p);
  s.loc = s.bsum + kMaxBlocks;
  s.acc = reinterpret_cast<uint2*>(s.loc + njobs);
  return s;
}

// A job's bytes: head (up to the first 16-byte boundary), np whole pieces at bulk, rest.
struct Geo {
  const uint8_t* bulk;
  uint64_t np;
  uint32_t head, rest;
};
__device__ __forceinline__ Geo job_geo(const void* data, uint64_t len) {
  const uint8_t* d = static_cast<const uint8_t*>(data);
  uint64_t head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;
  if (len < head) head = len;
  const uint64_t m = len - head;
  Geo g;
  g.bulk = d + head;
  g.np = m >> 4;
  g.head = (uint32_t)head;
  g.rest = (uint32_t)(m & 15);
  return g;
}
__device__ __forceinline__ uint64_t tiles_of(uint64_t np) { return (np + kBatchPieces - 1) / kBatchPieces; }

__device__ __forceinline__ uint32_t uni32(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  return ((uint64_t)uni32((uint32_t)(v >> 32)) << 32) | uni32((uint32_t)v);
}

// Exclusive prefix sum of v over the workgroup's 1024 lanes (wsum: kWaves LDS words); *total = the sum.
__device__ uint64_t block_scan_excl(uint64_t v, uint64_t* wsum, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint64_t o = __shfl_up(inc, off, 64);
    if (lane >= (uint32_t)off) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint64_t base = 0, tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < (uint32_t)kWaves; ++k) {
    const uint64_t s = wsum[k];
    if (k < wave) base += s;
    tot += s;
  }
  __syncthreads();  // wsum may be written again
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(kBatchLanes) void batch_prep_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                                 void* scratch) {
  __shared__ uint64_t wsum[kWaves];
  const Scratch S = scratch_of(scratch, njobs);
  const uint32_t j = blockIdx.x * kPrefixBlock + threadIdx.x;
  uint64_t t = 0;
  if (j < njobs) {
    const efes_job* jb = jobs + j;
    if (jb->sha1 == nullptr && jb->crc32 != nullptr) t = tiles_of(job_geo(jb->data, jb->length).np);
    S.acc[j] = make_uint2(0u, 0u);
  }
  uint64_t total;
  const uint64_t excl = block_scan_excl(t, wsum, &total);
  if (j < njobs) S.loc[j] = excl;
  if (threadIdx.x == 0) S.bsum[blockIdx.x] = total;
}

// LDS of the tile kernel: the slicing-by-4 tables in span_kernel's layout (entry e of table t, copy c
// at byte 256 e + 64 t + 4 c; lane j reads copy j mod 16 and visits the tables in the order
// (i + j / 16) mod 4, so no lookup instruction conflicts), the two stride operators, and the block
// offsets of the prefix sum.  80.3 KiB: one workgroup per CU.
constexpr int kCopies = 16;
struct BatchLDS {
  uint32_t lane_shift[4][256];  // Z^kLaneStride, byte-sliced
  uint32_t tile_shift[4][256];  // Z^kTileStride
  uint32_t slice[256][4][kCopies];
  uint64_t boff[kMaxBlocks];
  uint64_t wsum[kWaves];
  uint32_t wave_sum[2][kWaves];
};

// Raw CRC (from a zero register) of one 16-byte piece: line_raw of efes_crc_span.hip, four words.
__device__ __forceinline__ uint32_t piece_raw(const BatchLDS& L, uint32_t lb, const uint32_t (&sel)[4], v4u w) {
  const char* base = reinterpret_cast<const char*>(&L.slice);
  auto look = [&](uint32_t x, int i) {
    return *reinterpret_cast<const uint32_t*>(base + __builtin_amdgcn_perm(x, lb, sel[i]));
  };
  uint32_t x = w.x;
  uint32_t p = __builtin_amdgcn_bitop3_b32(look(x, 0), look(x, 1), look(x, 2), 0x96);
  x = __builtin_amdgcn_bitop3_b32(p, look(x, 3), w.y, 0x96);
  p = __builtin_amdgcn_bitop3_b32(look(x, 0), look(x, 1), look(x, 2), 0x96);
  x = __builtin_amdgcn_bitop3_b32(p, look(x, 3), w.z, 0x96);
  p = __builtin_amdgcn_bitop3_b32(look(x, 0), look(x, 1), look(x, 2), 0x96);
  x = __builtin_amdgcn_bitop3_b32(p, look(x, 3), w.w, 0x96);
  p = __builtin_amdgcn_bitop3_b32(look(x, 0), look(x, 1), look(x, 2), 0x96);
  return p ^ look(x, 3);
}

// Z^stride(v) ^ raw from a byte-sliced operator table.
__device__ __forceinline__ uint32_t shift_fold(const uint32_t (&s)[4][256], uint32_t v, uint32_t raw) {
  const uint32_t p = __builtin_amdgcn_bitop3_b32(s[0][v & 0xffu], s[1][(v >> 8) & 0xffu], s[2][(v >> 16) & 0xffu], 0x96);
  return __builtin_amdgcn_bitop3_b32(p, s[3][v >> 24], raw, 0x96);
}

// One tile of one job (wave-uniform): tile i of the job's nt, whose bulk holds np pieces.
struct TileDesc {
  uint32_t job;
  uint64_t i, nt, np;
  const uint8_t* bulk;
  uint8_t* dst;  // the copying pass: where bulk's bytes land (dst[job] + head), nullptr for a job that is not copied
};

struct BatchArgs {
  const efes_job* jobs;
  void* scratch;
  const Tables* tabs;
  const BatchTables* batch;
  uint32_t njobs, nblocks;
};
struct CopyArgs : BatchArgs {  // the copying tile pass (efes_crc32_copy)
  void* const* dsts;           // the call's pointer array, parallel to jobs
};

template <bool kCopy>
__device__ __forceinline__ void desc_of_job(const efes_job* __restrict__ jobs, void* const* __restrict__ dsts, uint32_t j,
                                            TileDesc& D) {
  const Geo g = job_geo(reinterpret_cast<const void*>(uni64(reinterpret_cast<uint64_t>(jobs[j].data))), uni64(jobs[j].length));
  D.job = j;
  D.i = 0;
  D.np = g.np;
  D.nt = tiles_of(g.np);
  D.bulk = g.bulk;
  D.dst = nullptr;
  if (kCopy) {
    uint8_t* o = reinterpret_cast<uint8_t*>(uni64(reinterpret_cast<uint64_t>(dsts[j])));
    if (o) D.dst = o + g.head;
  }
}

// The lane's pieces of tile D: piece 256 wave + 64 k + lane, zero where the bulk has ended.
__device__ __forceinline__ void load_tile(const TileDesc& D, uint32_t first, v4u (&w)[kPerLane]) {
  const uint64_t p0 = D.i * (uint64_t)kBatchPieces + first;
  const __attribute__((address_space(1))) v4u* src =
      (const __attribute__((address_space(1))) v4u*)D.bulk + p0;
#pragma unroll
  for (int k = 0; k < kPerLane; ++k) {
    v4u v = {0u, 0u, 0u, 0u};
    if (p0 + 64u * k < D.np) v = src[64 * k];
    w[k] = v;
  }
}

// Piece p of a job's bulk to its destination: one plain 16-byte store at any alignment (a wave writes
// 1 KiB contiguously).  Nontemporal stores were no faster (DESIGN.md §4 "Copy with CRC").
__device__ __forceinline__ void store_piece(uint8_t* dst, uint64_t p, v4u v) {
  *((__attribute__((address_space(1))) v4u_u*)dst + p) = v;
}

// The tile pass: batch_tile_kernel<false> is the pass of efes_crc32_batch and efes_crc32_chain.
// batch_tile_kernel<true> (efes_crc32_copy) also stores every piece it hashes to its job's destination,
// under the predicate that guards the piece's load, so the pieces load_tile zero-pads are never stored.
// Without kCopy nothing of dsts or TileDesc::dst is left.
template <bool kCopy>
__global__ __launch_bounds__(kBatchLanes) void batch_tile_kernel(const std::conditional_t<kCopy, CopyArgs, BatchArgs> a) {
  __shared__ __attribute__((aligned(16))) BatchLDS L;
  void* const* __restrict__ dsts = nullptr;
  if constexpr (kCopy) dsts = a.dsts;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const Scratch S = scratch_of(a.scratch, a.njobs);
  {  // tables into LDS: each slicing entry kCopies times, the two stride operators once
    uint4* dst = reinterpret_cast<uint4*>(&L.slice);
    for (uint32_t i = tid; i < sizeof(L.slice) / 16; i += kBatchLanes) {
      const uint32_t word = 4 * i;  // entry word >> 6, table (word >> 4) & 3
      const uint32_t v = a.tabs->slice8[(word >> 4) & 3u][word >> 6];
      dst[i] = make_uint4(v, v, v, v);
    }
    const uint32_t e = (tid & 255u) << (8 * (tid >> 8));
    L.lane_shift[tid >> 8][tid & 255u] = gf2_mulmod(a.batch->lane_stride_op, e);
    L.tile_shift[tid >> 8][tid & 255u] = gf2_mulmod(a.batch->tile_stride_op, e);
  }
  uint64_t total;
  {  // block offsets of the prefix sum, and the tile total
    const uint64_t v = tid < a.nblocks ? S.bsum[tid] : 0;
    L.boff[tid] = block_scan_excl(v, L.wsum, &total);
  }
  __syncthreads();
  const uint64_t G = gridDim.x, q = (total + G - 1) / G;
  const uint64_t t0 = (uint64_t)blockIdx.x * q;
  if (t0 >= total) return;  // uniform over the workgroup (an empty batch: every workgroup)
  const uint64_t t1 = t0 + q < total ? t0 + q : total;

  // excl(idx): tiles before job idx; past the last job, more than any tile index
  auto excl = [&](uint64_t idx) -> uint64_t {
    return idx < a.njobs ? S.loc[idx] + L.boff[idx / kPrefixBlock] : ~0ull;
  };
  TileDesc D;
  {  // the job of tile t0: the last block, then the last job of it, that starts at or before t0
    const uint32_t b = (uint32_t)__syncthreads_count(tid < a.nblocks && L.boff[tid] <= t0) - 1u;
    const uint64_t idx = (uint64_t)b * kPrefixBlock + tid;
    const uint32_t j = b * kPrefixBlock + (uint32_t)__syncthreads_count(excl(idx) <= t0) - 1u;
    desc_of_job<kCopy>(a.jobs, dsts, uni32(j), D);
    D.i = t0 - uni64(excl(D.job));
  }
  // The job of tile t (> D's tile), which is not in D's job: the last job behind D.job that starts at
  // or before t.  e = excl(base + lane), already loaded.
  auto next_job = [&](uint32_t base, uint64_t e, uint64_t t) -> uint32_t {
    for (;;) {
      const uint32_t cnt = (uint32_t)__popcll(__ballot(e <= t));
      if (cnt == 0u) return base < a.njobs ? base : a.njobs - 1u;  // not reached while loc[] is a prefix sum; stays in the array
      if (cnt < 64u) return base + cnt - 1u;
      base += 63u;  // 64 starts at or before t (jobs without tiles): go on from the last of them
      e = excl((uint64_t)base + lane);
    }
  };

  uint32_t lb = 0, sel[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t t = (uint32_t)(i + (int)(tid / 16)) & 3u;
    lb |= (64u * t + 4u * (tid % kCopies)) << (8 * i);
    sel[i] = 0x0C0C0000u | ((4u + 3u - t) << 8) | (uint32_t)i;
  }
  const uint32_t first = 256u * wave + lane;  // the lane's piece k = 0 of a tile

  v4u cur[kPerLane];
  load_tile(D, first, cur);
  bool have_next = t0 + 1 < t1;
  TileDesc N = D;
  if (have_next) {
    if (D.i + 1 < D.nt) {
      N.i = D.i + 1;
    } else {
      const uint32_t base = D.job + 1u;
      desc_of_job<kCopy>(a.jobs, dsts, next_job(base, excl((uint64_t)base + lane), t0 + 1), N);
    }
  }
  uint32_t acc = 0, parity = 0;
  for (uint64_t t = t0; t < t1; ++t) {
    // ---- issue: the next tile's bytes, and what locates the tile after it
    v4u nxt[kPerLane];
    if (have_next) load_tile(N, first, nxt);
    const bool have_next2 = t + 2 < t1;
    const bool same2 = N.i + 1 < N.nt;
    const uint32_t base2 = N.job + 1u;
    uint64_t e2 = 0;
    TileDesc spec = N;  // the job right behind N's, the usual successor
    if (have_next2 && !same2) {
      e2 = excl((uint64_t)base2 + lane);
      desc_of_job<kCopy>(a.jobs, dsts, base2 < a.njobs ? base2 : a.njobs - 1u, spec);
    }

    // ---- hash tile D from cur
    const uint64_t p0 = D.i * (uint64_t)kBatchPieces + first;
    uint32_t kv = 0;  // the lane's pieces in this tile (a prefix of k = 0..3)
#pragma unroll
    for (int k = 0; k < kPerLane; ++k) {
      if (p0 + 64u * k < D.np) {
        if (kCopy && D.dst) store_piece(D.dst, p0 + 64u * k, cur[k]);
        const uint32_t raw = piece_raw(L, lb, sel, cur[k]);
        acc = shift_fold(k == 0 ? L.tile_shift : L.lane_shift, acc, raw);
        kv = k + 1;
      }
    }

    // ---- the end of a run: D is its job's last tile, or the next tile does not continue the run
    const bool last = D.i + 1 == D.nt;
    const bool cont = !last && have_next && N.job == D.job && N.i + 1 != N.nt;
    if (!cont) {
      const uint64_t left = D.np - D.i * (uint64_t)kBatchPieces;
      const uint32_t in_tile = left < (uint64_t)kBatchPieces ? (uint32_t)left : (uint32_t)kBatchPieces;
      uint32_t c = 0;
      if (kv) c = gf2_mulmod(a.batch->piece_op[in_tile - 1u - (first + 64u * (kv - 1u))], acc);
      acc = 0;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) c ^= __shfl_xor(c, off, 64);
      if (lane == 0) L.wave_sum[parity][wave] = c;
      __syncthreads();
      if (tid == 0) {
        uint32_t x = 0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) x ^= L.wave_sum[parity][v];
        if (last) {
          atomicXor(&S.acc[D.job].y, x);
        } else {  // advance over the job's whole tiles behind this one, short of the last tile
          const uint64_t after = D.nt - 2 - D.i;
          x = gf2_mulmod(a.batch->tile_op[after % kBatchTileOps], x);
          if (after / kBatchTileOps) x = gf2_mulmod(xpow8n((after / kBatchTileOps) << 24, a.batch->x2n), x);
          atomicXor(&S.acc[D.job].x, x);
        }
      }
      parity ^= 1u;  // the next run's sums go to the other half: lane 0 may still be reading this one
    }

    // ---- resolve the tile after next
    TileDesc N2 = N;
    if (have_next2) {
      if (same2) {
        N2.i = N.i + 1;
      } else {
        const uint32_t j2 = next_job(base2, e2, t + 2);
        if (j2 == spec.job) N2 = spec;
        else desc_of_job<kCopy>(a.jobs, dsts, j2, N2);
      }
    }
    if (have_next) {
#pragma unroll
      for (int k = 0; k < kPerLane; ++k) cur[k] = nxt[k];
    }
    D = N;
    N = N2;
    have_next = have_next2;
  }
}

__device__ __forceinline__ uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }

__global__ __launch_bounds__(256) void batch_finish_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                           void* scratch, const Tables* __restrict__ tabs,
                                                           const BatchTables* __restrict__ batch) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= njobs) return;
  const efes_job jb = jobs[j];
  if (jb.sha1 != nullptr) {  // not a CRC-only job: reported, nothing of it touched
    if (jb.status) *jb.status = EFES_ERR_ARG;
    return;
  }
  const bool do_crc = jb.crc32 != nullptr;
  uint32_t crc = 0;
  if (do_crc) {
    const Scratch S = scratch_of(scratch, njobs);
    const uint32_t* t0 = tabs->slice8[0];
    const uint8_t* d = static_cast<const uint8_t*>(jb.data);
    const Geo g = job_geo(jb.data, jb.length);
    uint32_t r = (jb.flags & EFES_JOB_INIT) ? 0xFFFFFFFFu : ~jb.crc32->crc;  // crc32.go:123
    for (uint32_t i = 0; i < g.head; ++i) r = t0[(r ^ d[i]) & 0xffu] ^ (r >> 8);  // crc32.go:125
    const uint8_t* rest = g.bulk + 16 * g.np;
    uint32_t tail = 0;  // raw CRC of the rest bytes from a zero register
    for (uint32_t i = 0; i < g.rest; ++i) tail = t0[(tail ^ rest[i]) & 0xffu] ^ (tail >> 8);
    uint32_t bulk = 0;
    if (g.np) {
      const uint2 acc = S.acc[j];
      const uint64_t last_bytes = 16 * g.np - (tiles_of(g.np) - 1) * kTile;
      bulk = gf2_mulmod(xpow8n(last_bytes, batch->x2n), acc.x) ^ acc.y;
    }
    const uint64_t m = jb.length - g.head;
    crc = ~(gf2_mulmod(xpow8n(m, batch->x2n), r) ^ gf2_mulmod(xpow8n(g.rest, batch->x2n), bulk) ^ tail);
    if (!(jb.flags & EFES_JOB_SUM_ONLY)) jb.crc32->crc = crc;
  }
  if ((jb.flags & EFES_JOB_FINALIZE) && jb.sum) {  // SHA-1 Sum (none: zeros) then CRC-32 Sum, big-endian
    uint32_t* s = reinterpret_cast<uint32_t*>(jb.sum);
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = 0u;
    s[5] = bswap32(do_crc ? crc : 0u);
  }
  if (jb.status) *jb.status = EFES_OK;
}

// ---- chained jobs (efes_crc32_chain): prep and tile kernels as above, then map / carry / finish ----

// Both products a * b0 and a * b1 mod P in one pass: the product commutes, so the bits are taken from
// b0 and b1 and the one shifted operand, a, serves both (7 operations a step instead of gf2_mulmod's 10).
__device__ __forceinline__ void gf2_mulmod2(uint32_t a, uint32_t b0, uint32_t b1, uint32_t& p0, uint32_t& p1) {
  uint32_t q0 = 0, q1 = 0;
  for (int i = 0; i < 32; ++i) {
    q0 ^= a & (0u - ((b0 >> (31 - i)) & 1u));
    q1 ^= a & (0u - ((b1 >> (31 - i)) & 1u));
    a = (a >> 1) ^ (kPolyReflected & (0u - (a & 1u)));
  }
  p0 = q0;
  p1 = q1;
}

// What a job does to the pair (raw register r, bad bit): r -> m (x) r ^ b, bad -> (a & bad) | c.
// f holds a in bit 0 and c in bit 1.  A head has m = 0 and a = 0: whatever came before it is dropped.
struct Aff {
  uint32_t m, b, f;
};
constexpr uint32_t kAffPass = 1u, kAffBad = 2u;
__device__ __forceinline__ Aff aff_identity() { return Aff{1u << 31, 0u, kAffPass}; }
// hi after lo.
__device__ __forceinline__ Aff aff_compose(const Aff& hi, const Aff& lo) {
  Aff r;
  uint32_t pb;
  gf2_mulmod2(hi.m, lo.m, lo.b, r.m, pb);
  r.b = pb ^ hi.b;
  r.f = (hi.f & lo.f & kAffPass) | ((hi.f & kAffPass) ? (lo.f & kAffBad) : 0u) | (hi.f & kAffBad);
  return r;
}
__device__ __forceinline__ uint4 aff_pack(const Aff& e) { return make_uint4(e.m, e.b, e.f, 0u); }
__device__ __forceinline__ Aff aff_unpack(const uint4 v) { return Aff{v.x, v.y, v.z}; }

// Inclusive scan of e over `width` (<= 64) lanes of a wave, in job order.
__device__ __forceinline__ Aff wave_scan_incl(Aff e, uint32_t lane, int width) {
  for (int off = 1; off < width; off <<= 1) {
    Aff lo;
    lo.m = __shfl_up(e.m, off, 64);
    lo.b = __shfl_up(e.b, off, 64);
    lo.f = __shfl_up(e.f, off, 64);
    if (lane >= (uint32_t)off) e = aff_compose(e, lo);
  }
  return e;
}

// Inclusive scan over the workgroup's lanes (a multiple of 64, up to 1024): wave shuffles, then the
// wave totals through LDS (wave 0 scans them).  Every lane of the workgroup calls it.
__device__ Aff block_scan_aff(Aff e, uint4* wtot) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
  e = wave_scan_incl(e, lane, 64);
  if (nwaves == 1u) return e;  // uniform over the workgroup
  if (lane == 63u) wtot[wave] = aff_pack(e);
  __syncthreads();
  if (wave == 0u) {
    const Aff t = wave_scan_incl(lane < nwaves ? aff_unpack(wtot[lane]) : aff_identity(), lane, kWaves);
    if (lane < nwaves) wtot[lane] = aff_pack(t);
  }
  __syncthreads();
  if (wave) e = aff_compose(e, aff_unpack(wtot[wave - 1u]));
  return e;
}

// Chain scratch: the batch scratch | elem[njobs] | btot[blocks of kPrefixBlock jobs], 16 bytes each.
struct ChainScratch {
  uint4* elem;
  uint4* btot;
};
__host__ __device__ inline size_t batch_scratch_size(uint32_t njobs) {
  return sizeof(uint64_t) * kMaxBlocks + (sizeof(uint64_t) + sizeof(uint2)) * (size_t)njobs;
}
__host__ __device__ inline ChainScratch chain_scratch_of(void* p, uint32_t njobs) {
  static_assert((sizeof(uint64_t) * kMaxBlocks) % 16 == 0 && sizeof(uint64_t) + sizeof(uint2) == 16, "elem[] stays 16-byte aligned");
  ChainScratch c;
  c.elem = reinterpret_cast<uint4*>(static_cast<char*>(p) + batch_scratch_size(njobs));
  c.btot = c.elem + njobs;
  return c;
}

// A job with EFES_JOB_CHAIN behind the job (prev_crc32, prev_flags), j > 0: not a Write into that job's state.
__device__ __forceinline__ bool follower_bad(const efes_job& jb, const efes_crc32_state* prev_crc32, uint32_t prev_flags) {
  return jb.sha1 != nullptr || jb.crc32 == nullptr || jb.crc32 != prev_crc32 ||
         (jb.flags & (EFES_JOB_INIT | EFES_JOB_SUM_ONLY)) != 0u || (prev_flags & EFES_JOB_SUM_ONLY) != 0u;
}

// The map pass.  kCopy (efes_crc32_copy): the lane also lands the job's head and rest bytes, which it
// reads byte by byte anyway, at dsts[j] and behind the bulk's pieces there.
template <bool kCopy>
__device__ __forceinline__ void map_pass(const efes_job* __restrict__ jobs, uint32_t njobs, void* scratch,
                                         const Tables* __restrict__ tabs, const BatchTables* __restrict__ batch,
                                         void* const* __restrict__ dsts, uint4* wtot) {
  const uint32_t j = blockIdx.x * kPrefixBlock + threadIdx.x;
  const ChainScratch C = chain_scratch_of(scratch, njobs);
  Aff e = aff_identity();  // the lanes past the array
  if (j < njobs) {
    const efes_job jb = jobs[j];
    const bool chained = (jb.flags & EFES_JOB_CHAIN) != 0u;
    bool bad = jb.sha1 != nullptr;
    if (chained) bad = j == 0u || follower_bad(jb, jobs[j - 1u].crc32, jobs[j - 1u].flags);
    e = Aff{0u, 0u, (chained ? kAffPass : 0u) | (bad ? kAffBad : 0u)};
    if (!bad && jb.crc32 != nullptr) {
      const Scratch S = scratch_of(scratch, njobs);
      const uint32_t* t0 = tabs->slice8[0];
      const uint8_t* d = static_cast<const uint8_t*>(jb.data);
      const Geo g = job_geo(jb.data, jb.length);
      uint8_t* o = kCopy ? static_cast<uint8_t*>(dsts[j]) : nullptr;
      // The register after the head bytes: from the in-state for a head (crc32.go:123), whose map then
      // forgets what came before (m = 0), from zero for a follower.
      uint32_t r = 0;
      if (!chained) r = (jb.flags & EFES_JOB_INIT) ? 0xFFFFFFFFu : ~jb.crc32->crc;
      for (uint32_t i = 0; i < g.head; ++i) {
        const uint8_t c = d[i];
        if (kCopy && o) o[i] = c;
        r = t0[(r ^ c) & 0xffu] ^ (r >> 8);  // crc32.go:125
      }
      const uint32_t behind_head = xpow8n(jb.length - g.head, batch->x2n);
      if (r) r = gf2_mulmod(behind_head, r);
      uint32_t t = 0;  // the bulk's raw CRC from the two accumulators, as batch_finish_kernel combines them
      if (g.np) {
        const uint2 acc = S.acc[j];
        const uint64_t nt = tiles_of(g.np);
        t = acc.y;
        if (nt > 1) t ^= gf2_mulmod(xpow8n(16 * g.np - (nt - 1) * kTile, batch->x2n), acc.x);
      }
      // one table step is x^8: going on byte-wise from t gives Z^rest(bulk) ^ raw(rest)
      const uint8_t* rest = g.bulk + 16 * g.np;
      uint8_t* orest = o ? o + g.head + 16 * g.np : nullptr;
      for (uint32_t i = 0; i < g.rest; ++i) {
        const uint8_t c = rest[i];
        if (kCopy && o) orest[i] = c;
        t = t0[(t ^ c) & 0xffu] ^ (t >> 8);
      }
      e.b = r ^ t;
      if (chained) {  // m = x^(8 length): the head's zero bytes applied to x^(8 (length - head))
        e.m = behind_head;
        for (uint32_t i = 0; i < g.head; ++i) e.m = t0[e.m & 0xffu] ^ (e.m >> 8);
      }
    }
  }
  e = block_scan_aff(e, wtot);
  if (j < njobs) C.elem[j] = aff_pack(e);
  if (threadIdx.x == kPrefixBlock - 1u) C.btot[blockIdx.x] = aff_pack(e);
}

__global__ __launch_bounds__(kBatchLanes) void chain_map_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                                void* scratch, const Tables* __restrict__ tabs,
                                                                const BatchTables* __restrict__ batch) {
  __shared__ uint4 wtot[kWaves];
  map_pass<false>(jobs, njobs, scratch, tabs, batch, nullptr, wtot);
}

__global__ __launch_bounds__(kBatchLanes) void copy_map_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                               void* scratch, const Tables* __restrict__ tabs,
                                                               const BatchTables* __restrict__ batch,
                                                               void* const* __restrict__ dsts) {
  __shared__ uint4 wtot[kWaves];
  map_pass<true>(jobs, njobs, scratch, tabs, batch, dsts, wtot);
}

// btot[k] becomes the map of the blocks 0..k together.  One workgroup of at least nblocks lanes.
__global__ __launch_bounds__(kBatchLanes) void chain_carry_kernel(uint32_t njobs, uint32_t nblocks, void* scratch) {
  __shared__ uint4 wtot[kWaves];
  const ChainScratch C = chain_scratch_of(scratch, njobs);
  const uint32_t k = threadIdx.x;
  const Aff e = block_scan_aff(k < nblocks ? aff_unpack(C.btot[k]) : aff_identity(), wtot);
  if (k < nblocks) C.btot[k] = aff_pack(e);
}

__global__ __launch_bounds__(256) void chain_finish_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                           void* scratch) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= njobs) return;
  const ChainScratch C = chain_scratch_of(scratch, njobs);
  const efes_job jb = jobs[j];
  Aff e = aff_unpack(C.elem[j]);
  const uint32_t blk = j / kPrefixBlock;
  if (blk) {  // nothing comes before job 0: register 0, not bad
    const Aff carry = aff_unpack(C.btot[blk - 1u]);
    e.b ^= gf2_mulmod(e.m, carry.b);
    e.f |= (e.f & kAffPass) ? (carry.f & kAffBad) : 0u;
  }
  if (e.f & kAffBad) {  // not a Write into its chain's state: reported, nothing of it touched
    if (jb.status) *jb.status = EFES_ERR_ARG;
    return;
  }
  const bool do_crc = jb.crc32 != nullptr;
  const uint32_t crc = ~e.b;  // the CRC after this job's Write
  bool tail = j + 1u == njobs;
  if (!tail) {
    const efes_job nx = jobs[j + 1u];
    tail = !(nx.flags & EFES_JOB_CHAIN) || follower_bad(nx, jb.crc32, jb.flags);
  }
  if (do_crc && tail && !(jb.flags & EFES_JOB_SUM_ONLY)) jb.crc32->crc = crc;
  if ((jb.flags & EFES_JOB_FINALIZE) && jb.sum) {  // as batch_finish_kernel
    uint32_t* s = reinterpret_cast<uint32_t*>(jb.sum);
#pragma unroll
    for (int k = 0; k < 5; ++k) s[k] = 0u;
    s[5] = bswap32(do_crc ? crc : 0u);
  }
  if (jb.status) *jb.status = EFES_OK;
}

}  // namespace

void build_batch_tables(BatchTables* t) {
  t->x2n[0] = 1u << 30;  // x^1
  for (int k = 1; k < 32; ++k) t->x2n[k] = gf2_mulmod(t->x2n[k - 1], t->x2n[k - 1]);
  const uint32_t piece = xpow8n(16), tile = xpow8n(kTile);
  t->piece_op[0] = t->tile_op[0] = 1u << 31;  // x^0
  for (int i = 1; i < kBatchPieces; ++i) t->piece_op[i] = gf2_mulmod(piece, t->piece_op[i - 1]);
  for (int i = 1; i < kBatchTileOps; ++i) t->tile_op[i] = gf2_mulmod(tile, t->tile_op[i - 1]);
  t->lane_stride_op = xpow8n(kLaneStride);
  t->tile_stride_op = xpow8n(kTileStride);
}

size_t crc_batch_scratch_bytes(uint32_t njobs) {
  if (njobs == 0 || njobs > EFES_CRC_BATCH_MAX_JOBS) return 0;
  return batch_scratch_size(njobs);
}

// The two launches every path starts with: tiles per job, then the tiles (dsts: the copying tile pass).
static hipError_t launch_prep_and_tiles(const efes_job* jobs, uint32_t njobs, void* scratch, const Tables* tabs,
                                        const BatchTables* batch, int cus, hipStream_t s, void* const* dsts = nullptr) {
  const uint32_t nblocks = (njobs + kPrefixBlock - 1) / kPrefixBlock;
  clear_last_error();
  hipLaunchKernelGGL(batch_prep_kernel, dim3(nblocks), dim3(kBatchLanes), 0, s, jobs, njobs, scratch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  CopyArgs a{};
  a.dsts = dsts;
  a.jobs = jobs;
  a.scratch = scratch;
  a.tabs = tabs;
  a.batch = batch;
  a.njobs = njobs;
  a.nblocks = nblocks;
  clear_last_error();
  const dim3 grid((uint32_t)(cus > 0 ? cus : 256));
  if (dsts) hipLaunchKernelGGL(batch_tile_kernel<true>, grid, dim3(kBatchLanes), 0, s, a);
  else hipLaunchKernelGGL(batch_tile_kernel<false>, grid, dim3(kBatchLanes), 0, s, static_cast<const BatchArgs&>(a));
  return hipGetLastError();
}

hipError_t launch_crc_batch(const efes_job* jobs, uint32_t njobs, void* scratch, const Tables* tabs,
                            const BatchTables* batch, int cus, hipStream_t s) {
  hipError_t e = launch_prep_and_tiles(jobs, njobs, scratch, tabs, batch, cus, s);
  if (e != hipSuccess) return e;
  clear_last_error();
  hipLaunchKernelGGL(batch_finish_kernel, dim3((njobs + 255u) / 256u), dim3(256), 0, s, jobs, njobs, scratch, tabs, batch);
  return hipGetLastError();
}

size_t crc_chain_scratch_bytes(uint32_t njobs) {
  if (njobs == 0 || njobs > EFES_CRC_BATCH_MAX_JOBS) return 0;
  const size_t nblocks = (njobs + kPrefixBlock - 1) / kPrefixBlock;
  return batch_scratch_size(njobs) + sizeof(uint4) * ((size_t)njobs + nblocks);
}

// efes_crc32_chain, and with dsts efes_crc32_copy: the copying tile and map passes in place of the plain ones.
static hipError_t launch_chain(const efes_job* jobs, void* const* dsts, uint32_t njobs, void* scratch, const Tables* tabs,
                               const BatchTables* batch, int cus, hipStream_t s) {
  const uint32_t nblocks = (njobs + kPrefixBlock - 1) / kPrefixBlock;
  hipError_t e = launch_prep_and_tiles(jobs, njobs, scratch, tabs, batch, cus, s, dsts);
  if (e != hipSuccess) return e;
  clear_last_error();
  if (dsts) hipLaunchKernelGGL(copy_map_kernel, dim3(nblocks), dim3(kBatchLanes), 0, s, jobs, njobs, scratch, tabs, batch, dsts);
  else hipLaunchKernelGGL(chain_map_kernel, dim3(nblocks), dim3(kBatchLanes), 0, s, jobs, njobs, scratch, tabs, batch);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (nblocks > 1) {  // one block of jobs has no carry to take
    clear_last_error();
    hipLaunchKernelGGL(chain_carry_kernel, dim3(1), dim3((nblocks + 63u) / 64u * 64u), 0, s, njobs, nblocks, scratch);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  clear_last_error();
  hipLaunchKernelGGL(chain_finish_kernel, dim3((njobs + 255u) / 256u), dim3(256), 0, s, jobs, njobs, scratch);
  return hipGetLastError();
}

hipError_t launch_crc_chain(const efes_job* jobs, uint32_t njobs, void* scratch, const Tables* tabs,
                            const BatchTables* batch, int cus, hipStream_t s) {
  return launch_chain(jobs, nullptr, njobs, scratch, tabs, batch, cus, s);
}

hipError_t launch_crc_copy(const efes_job* jobs, void* const* dsts, uint32_t njobs, void* scratch, const Tables* tabs,
                           const BatchTables* batch, int cus, hipStream_t s) {
  return launch_chain(jobs, dsts, njobs, scratch, tabs, batch, cus, s);
}

}  // namespace efes
