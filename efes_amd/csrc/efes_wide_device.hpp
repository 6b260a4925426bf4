// efes_wide_device.hpp -- device helpers shared by the translation units that hold kernels: the CRC and
// load helpers, the WIDE shape's block step and bulk loop (wide_kernel in efes_kernels.hip, the wide chain walk
// in efes_chain_wide.hip) and the layout of the chain calls' scratch.  Everything here is __forceinline__ or a
// constant, so each translation unit compiles its own copy into its own kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "efes_internal.hpp"
#include "sha1_device.hpp"

namespace efes {

// ------------------------------------------------------------------ CRC-32 helpers
// Raw (register-level) reflected CRC: Go's update is ~raw(~crc, p) (crc32.go:123,127,155,165).
__device__ __forceinline__ uint32_t crc_byte(const uint32_t* __restrict__ t0, uint32_t crc, uint32_t b) {
  return t0[(crc ^ b) & 0xffu] ^ (crc >> 8);  // crc32.go:125
}

__device__ __forceinline__ uint32_t crc_shift(const uint32_t (&s)[4][256], uint32_t v) {
  return s[0][v & 0xffu] ^ s[1][(v >> 8) & 0xffu] ^ s[2][(v >> 16) & 0xffu] ^ s[3][v >> 24];
}

// Slicing-by-8 over 64 bytes held as 16 little-endian words (crc32.go:157-161).
__device__ __forceinline__ uint32_t crc_words_raw(const uint32_t (&t)[8][256], uint32_t crc, const uint32_t (&le)[16]) {
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const uint32_t hi = le[2 * s + 1];
    crc ^= le[2 * s];
    // eight lookups folded with three-input XORs (v_bitop3_b32 0x96): 4 VALU instead of 7
    const uint32_t a = __builtin_amdgcn_bitop3_b32(t[0][hi >> 24], t[1][(hi >> 16) & 0xffu], t[2][(hi >> 8) & 0xffu], 0x96);
    const uint32_t b = __builtin_amdgcn_bitop3_b32(t[3][hi & 0xffu], t[4][crc >> 24], t[5][(crc >> 16) & 0xffu], 0x96);
    crc = __builtin_amdgcn_bitop3_b32(a, b, t[6][(crc >> 8) & 0xffu] ^ t[7][crc & 0xffu], 0x96);
  }
  return crc;
}

// __builtin_amdgcn_readfirstlane returns int: go through uint32_t so the low half of a
// 64-bit value is zero-extended (a sign-extended low half corrupts pointers >= 2^31).
__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  return (uint64_t)uniform32((uint32_t)v) | ((uint64_t)uniform32((uint32_t)(v >> 32)) << 32);
}

// Orders this wave's LDS stores before its later LDS loads from other lanes.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Big-endian word k (bytes 4k..4k+3) of a byte array in LDS.
__device__ __forceinline__ uint32_t be_word_lds(const uint8_t* b, int k) {
  return (uint32_t)b[4 * k] << 24 | (uint32_t)b[4 * k + 1] << 16 | (uint32_t)b[4 * k + 2] << 8 | b[4 * k + 3];
}

// Message bytes are always device global memory: address-space-1 pointers make the compiler
// emit global_load (counted by vmcnt only) instead of flat_load, which also counts in
// lgkmcnt and would make every LDS wait of the chain wait for the in-flight prefetch too.
#define EFES_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ const EFES_GLOBAL T* gptr(const T* p) {
  return (const EFES_GLOBAL T*)p;
}
__device__ __forceinline__ uint32_t ldg_u8(const uint8_t* p) { return *gptr(p); }

// Load 64 bytes at an arbitrary device address as 16 little-endian words.
// kAligned16: the address is 16-byte aligned (4 x global_load_dwordx4).
// Otherwise: 16 (or 17) naturally aligned dword loads funnel-shifted by v_alignbyte.  The
// 17th dword is loaded only when the block is misaligned, and then it holds a byte of the
// block, so it never touches a page the block does not touch.
template <bool kAligned16>
__device__ __forceinline__ void load_block_le(const uint8_t* src, uint32_t (&le)[16]) {
  if constexpr (kAligned16) {
    typedef uint32_t v4u __attribute__((ext_vector_type(4)));
    const EFES_GLOBAL v4u* s = gptr(reinterpret_cast<const v4u*>(src));
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const v4u v = s[q];
      le[4 * q] = v.x; le[4 * q + 1] = v.y; le[4 * q + 2] = v.z; le[4 * q + 3] = v.w;
    }
  } else {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    const EFES_GLOBAL uint32_t* s = gptr(reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3));
    const uint32_t sh = (uint32_t)(a & 3);
    uint32_t d[17];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = s[k];
    d[16] = sh ? s[16] : 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) le[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], sh);
  }
}

// ------------------------------------------------------------------ WIDE shape: constants, block step, bulk loop
constexpr int kWideWaves = 4;    // waves per workgroup per SIMD-wave (one per SIMD)
constexpr int kWideMaxWps = 3;   // waves per SIMD that fit (132 VGPRs)
constexpr int kXStride = 68;

// WIDE's CRC tables in LDS: the position tables (crc_issue below).
using WideCrcTab = uint32_t[64][256];

struct WideLDS {
  WideCrcTab crc;  // PosTables (64 KiB)
  uint32_t prog[kWideWaves * kWideMaxWps];  // blocks done by each wave of the workgroup
};
// The byte-wise head/tail: pos[63][b] (byte b, no byte after it) is IEEETable[b] (crc32.go:125).
__device__ __forceinline__ const uint32_t* wide_t0(const WideLDS& L) { return L.crc[63]; }
__device__ __forceinline__ const uint4* wide_tab_src(const Tables* tabs) {
  return reinterpret_cast<const uint4*>(tabs + 1);  // PosTables follow Tables (efes_ctx_create)
}

// The priority of wave w from its SIMD siblings' progress (w % 4, w % 4 + 4, ...): the furthest
// behind gets 3, the furthest ahead 0, the rest 1.  Wave-uniform; `b` = blocks this wave has done.
__device__ __forceinline__ void wide_pace(uint32_t* prog, uint32_t w, uint32_t nw, uint32_t b) {
  if (nw <= kWideWaves) return;  // one wave per SIMD: nothing to share
  __builtin_amdgcn_sched_barrier(0);
  if ((threadIdx.x & 63) == 0) __atomic_store_n(&prog[w], b, __ATOMIC_RELAXED);
  uint32_t lo = 0xffffffffu, hi = 0;
  for (uint32_t v = w & 3; v < nw; v += kWideWaves) {
    if (v == w) continue;
    const uint32_t o = __atomic_load_n(&prog[v], __ATOMIC_RELAXED);
    lo = o < lo ? o : lo;
    hi = o > hi ? o : hi;
  }
  lo = uniform32(lo);
  hi = uniform32(hi);
  if (b <= lo) __builtin_amdgcn_s_setprio(3);
  else if (b >= hi) __builtin_amdgcn_s_setprio(0);
  else __builtin_amdgcn_s_setprio(1);
  __builtin_amdgcn_sched_barrier(0);
}

// Byte i of the padded final stream x[:nxf] || 0x80 || 0.. || BE64(bits), length T.
__device__ __forceinline__ uint32_t fin_byte(const uint8_t* xl, uint32_t i, uint32_t nxf, uint32_t T, uint64_t bits) {
  if (i < nxf) return xl[i];
  if (i == nxf) return 0x80u;
  if (i >= T - 8) return (uint32_t)(bits >> (56 - 8 * (i - (T - 8)))) & 0xffu;
  return 0u;
}

// Whole blocks of one lane's message, software-pipelined: the next block is in flight while
// the current one is compressed (a lone uncoalesced 64-B load per lane would otherwise expose
// the full memory latency every block).  kSha/kCrc are wave-uniform template flags, so CRC
// lookups and SHA-1 rounds share one basic block; a lane that needs only one of the two
// computes both and never stores the other.  Lanes run their own trip counts; with jobs
// sorted by length the lanes of a wave finish together.

// The block's raw CRC from the position tables (pos[o][b]: the register after a 64-byte block
// whose only nonzero byte is b at offset o; efes_internal.hpp): crc32.go:153-169's slicing over
// the whole block at once.  The register is linear, so the new register is the XOR of 64
// lookups, and only the first four (bytes 0..3 XOR the old register, crc32.go:157) depend on the
// previous block.  Split in eight groups of eight bytes (LE words 2S, 2S+1): a group's lookups are
// issued first, the XORs that fold them into the running value come five SHA-1 rounds later.
// 97 VALU per block (64 lookup addresses, 1 + 32 XORs) against 112 for slicing-by-8's eight
// dependent steps (round 3 A/B, profiles/r03_wide_crc_ab/).
struct CrcPending {
  uint32_t v[8];
};
template <int S>
__device__ __forceinline__ void crc_issue(const WideCrcTab& t, uint32_t crc, const uint32_t (&le)[16], CrcPending& p) {
  const uint32_t lo = S == 0 ? crc ^ le[0] : le[2 * S];
  const uint32_t hi = le[2 * S + 1];
  constexpr int o = 8 * S;
  p.v[0] = t[o + 0][lo & 0xffu]; p.v[1] = t[o + 1][(lo >> 8) & 0xffu]; p.v[2] = t[o + 2][(lo >> 16) & 0xffu];
  p.v[3] = t[o + 3][lo >> 24]; p.v[4] = t[o + 4][hi & 0xffu]; p.v[5] = t[o + 5][(hi >> 8) & 0xffu];
  p.v[6] = t[o + 6][(hi >> 16) & 0xffu]; p.v[7] = t[o + 7][hi >> 24];
}
// Group S's eight values folded into the running value `acc` (group 0 starts it).
template <int S>
__device__ __forceinline__ uint32_t crc_combine(const CrcPending& p, uint32_t acc) {
  const uint32_t a = __builtin_amdgcn_bitop3_b32(p.v[0], p.v[1], p.v[2], 0x96);
  const uint32_t b = __builtin_amdgcn_bitop3_b32(p.v[3], p.v[4], p.v[5], 0x96);
  if constexpr (S == 0) return __builtin_amdgcn_bitop3_b32(a, b, p.v[6] ^ p.v[7], 0x96);
  const uint32_t c = __builtin_amdgcn_bitop3_b32(acc, a, b, 0x96);
  return __builtin_amdgcn_bitop3_b32(c, p.v[6], p.v[7], 0x96);
}

// 80 inline SHA-1 rounds with the 8 CRC groups of the same block woven in: group k's lookups are
// issued after round 10k+4 and combined after round 10k+9, so the LDS latency of the lookups is
// covered by SHA-1 rounds.  Scheduling barriers every five rounds keep the compiler from
// regrouping the CRC groups into back-to-back lookup/wait clusters.  `crc` is the register
// before the block until group 0 is issued, the running value after.
template <int R, bool kSha, bool kCrc>
struct WideRounds {
  __device__ __forceinline__ static void run(uint32_t (&s)[5], uint32_t (&w)[16], const WideCrcTab& t, uint32_t& crc,
                                             const uint32_t (&le)[16], CrcPending& p) {
    if constexpr (kSha) round_inline<R>(s, w);
    if constexpr (kCrc && R % 10 == 4) crc_issue<R / 10>(t, crc, le, p);
    if constexpr (kCrc && R % 10 == 9) {
      crc = crc_combine<R / 10>(p, crc);
      // Pins the fold here: the 64-term XOR is otherwise reassociated into one tree at the end of
      // the block, with all 64 lookups live at once (168 VGPRs and spills).
      asm volatile("" : "+v"(crc));
    }
    if constexpr (kSha && kCrc && R % 5 == 4) __builtin_amdgcn_sched_barrier(0);
    WideRounds<R + 1, kSha, kCrc>::run(s, w, t, crc, le, p);
  }
};
template <bool kSha, bool kCrc>
struct WideRounds<80, kSha, kCrc> {
  __device__ __forceinline__ static void run(uint32_t (&)[5], uint32_t (&)[16], const WideCrcTab&, uint32_t&,
                                             const uint32_t (&)[16], CrcPending&) {}
};

// One block of one lane's message; `live` lanes (b < their own block count) commit the result.
template <bool kSha, bool kCrc>
__device__ __forceinline__ void wide_step(const uint32_t (&le)[16], const WideCrcTab& t, uint32_t (&h)[5],
                                          uint32_t& crc_raw, bool live) {
  uint32_t w[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) w[k] = bswap(le[k]);
  uint32_t s[5] = {h[0], h[1], h[2], h[3], h[4]};
  uint32_t c = crc_raw;
  CrcPending p;
  WideRounds<0, kSha, kCrc>::run(s, w, t, c, le, p);
  if constexpr (kSha) {
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = live ? h[k] + s[k] : h[k];
  }
  if constexpr (kCrc) crc_raw = live ? c : crc_raw;
}

// Whole blocks of one lane's message: block b is hashed (SHA-1 rounds and CRC steps woven
// together) while the next blocks are in flight (three 16-word buffers, the loop unrolled so the
// buffers keep their registers).  Two phases:
//  * uniform: while every lane of the wave still has the blocks being hashed and prefetched
//    (b+5 < nmin, the wave's shortest message), loads are unconditional, a whole 128-B line (two
//    blocks) at a time, and every lane commits -- no per-lane selects (8 VALU per block fewer
//    than the ragged phase);
//  * ragged: up to the wave's longest message (`nmax`, uniform), so the loads stay
//    unconditional and the compiler's vmcnt waits exact; lanes past their own last block
//    load a harmless `dummy` block and do not commit.
// kSha/kCrc are wave-uniform template flags; a lane that needs only one of the two computes
// both and never stores the other.  Jobs sorted by length keep the lanes of a wave equally long.
template <bool kAligned16, bool kSha, bool kCrc>
__device__ __forceinline__ void wide_bulk(const uint8_t* q, uint64_t nbulk, uint64_t nmin, uint64_t nmax,
                                          const uint8_t* dummy, const WideCrcTab& t, uint32_t (&h)[5],
                                          uint32_t& crc_raw, uint32_t* prog, uint32_t w, uint32_t nw) {
  auto src = [&](uint64_t b) { return b < nbulk ? q + 64 * b : dummy; };
  uint32_t A[16], B[16], C[16];
  if (nmax == 0) return;
  load_block_le<kAligned16>(src(0), A);
  load_block_le<kAligned16>(src(1), B);
  uint64_t b = 0;
  // Uniform phase (blocks b..b+5 exist in every lane), a 128-B line at a time: the two blocks of a
  // line are loaded back to back (eight dwordx4), one block-time before the first is hashed.  A
  // lane's blocks loaded one at a time, a block apart (the A/B build below), fetched 14.5 % more
  // than the message from HBM (FETCH_SIZE x 2, calibrated on this access pattern with
  // tools/microbench/mb_wide_fetch: profiles/r04_fetch/): the second half of a line was often
  // evicted from L2 before the lane came back for it.  A holds the even block, B / C the odd one.
  for (; b + 5 < nmin; b += 4) {
    if (b % 32 == 0) wide_pace(prog, w, nw, (uint32_t)b);  // every 32 blocks (profiles/r05_wide_pace_ab/)
    const uint8_t* qb = q + 64 * b;
    wide_step<kSha, kCrc>(A, t, h, crc_raw, true);
    load_block_le<kAligned16>(qb + 128, A);
    load_block_le<kAligned16>(qb + 192, C);
    wide_step<kSha, kCrc>(B, t, h, crc_raw, true);
    wide_step<kSha, kCrc>(A, t, h, crc_raw, true);
    load_block_le<kAligned16>(qb + 256, A);
    load_block_le<kAligned16>(qb + 320, B);
    wide_step<kSha, kCrc>(C, t, h, crc_raw, true);
  }
  // ragged phase (A, B hold blocks b, b+1 or the dummy), paced at its start and every 6 blocks
  // (counted from the start: b enters at a multiple of 4, so b % 6 alone could skip every pace)
  for (const uint64_t b_ragged = b; b < nmax; b += 3) {
    if ((b - b_ragged) % 6 == 0) wide_pace(prog, w, nw, (uint32_t)b);
    load_block_le<kAligned16>(src(b + 2), C);
    wide_step<kSha, kCrc>(A, t, h, crc_raw, b < nbulk);
    if (b + 1 >= nmax) break;
    load_block_le<kAligned16>(src(b + 3), A);
    wide_step<kSha, kCrc>(B, t, h, crc_raw, b + 1 < nbulk);
    if (b + 2 >= nmax) break;
    load_block_le<kAligned16>(src(b + 4), B);
    wide_step<kSha, kCrc>(C, t, h, crc_raw, b + 2 < nbulk);
  }
}
template <bool kAligned16>
__device__ __forceinline__ void wide_bulk_any(const uint8_t* q, uint64_t nbulk, uint64_t nmin, uint64_t nmax,
                                              const uint8_t* dummy, bool any_sha, bool any_crc,
                                              const WideCrcTab& t, uint32_t (&h)[5], uint32_t& crc_raw,
                                              uint32_t* prog, uint32_t w, uint32_t nw) {
  if (any_sha && any_crc) wide_bulk<kAligned16, true, true>(q, nbulk, nmin, nmax, dummy, t, h, crc_raw, prog, w, nw);
  else if (any_sha) wide_bulk<kAligned16, true, false>(q, nbulk, nmin, nmax, dummy, t, h, crc_raw, prog, w, nw);
  else if (any_crc) wide_bulk<kAligned16, false, true>(q, nbulk, nmin, nmax, dummy, t, h, crc_raw, prog, w, nw);
}

// Wave-wide minimum of a per-lane 64-bit value over the lanes where `use` holds (uniform
// result; ~0 when no lane does).
__device__ __forceinline__ uint64_t wave_min64(uint64_t v, bool use) {
  v = use ? v : ~0ull;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, k);
    v = o < v ? o : v;
  }
  return uniform64(v);
}

// Wave-wide maximum of a per-lane 64-bit value (uniform result).
__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, k);
    v = o > v ? o : v;
  }
  return uniform64(v);
}

// LDS of one CU on gfx950; an exclusive launch asks for all of it per workgroup.
constexpr size_t kCuLds = 160 * 1024;

// ------------------------------------------------------------------ scratch of the chain calls (efes_hash_chain)
constexpr uint32_t kChainBlock = 1024;  // jobs per block of the head count
constexpr uint32_t kChainMaxBlocks = EFES_HASH_CHAIN_MAX_JOBS / kChainBlock;
static_assert(kChainMaxBlocks <= kChainBlock, "one lane per block count in hash_chain_list_kernel");

// Scratch: ctl (16 bytes) | bsum[kChainMaxBlocks] | loc[njobs] | heads[njobs], 32-bit words.
struct ChainCtl {
  uint32_t count;   // chains of this call (hash_chain_list_kernel)
  uint32_t ticket;  // next chain to take (zeroed by hash_chain_mark_kernel on every call)
  uint32_t pad[2];
};
struct HashChainScratch {
  ChainCtl* ctl;
  uint32_t* bsum;
  uint32_t* loc;
  uint32_t* heads;
};
__host__ __device__ inline HashChainScratch hash_chain_scratch_of(void* p, uint32_t njobs) {
  HashChainScratch s;
  s.ctl = static_cast<ChainCtl*>(p);
  s.bsum = reinterpret_cast<uint32_t*>(s.ctl + 1);
  s.loc = s.bsum + kChainMaxBlocks;
  s.heads = s.loc + njobs;
  return s;
}

}  // namespace efes
