// efes_chain_wide_device.hpp -- what the two translation units of the wide chain walk share beside its body
// (efes_chain_wide_body.inc): the stores and the bulk loop of the copying walk (efes_hash_chain_wide_copy in
// efes_chain_wide_copy.hip) and the launcher of both (efes_hash_chain_wide in efes_chain_wide.hip).  Everything
// here is __forceinline__ or a template, so each translation unit compiles its own copy into its own kernels,
// and efes_kernels.hip, which does not include this file, is compiled from the text it always had.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>

#include "efes_internal.hpp"
#include "sha1_device.hpp"
#include "efes_wide_device.hpp"

namespace efes {

static_assert(sizeof(WideLDS) + 64 * kWideWaves * kXStride > kCuLds / 2 &&
                  sizeof(WideLDS) + 64 * kWideWaves * kWideMaxWps * kXStride <= kCuLds,
              "one wide-walk workgroup per CU at every wps");

// ------------------------------------------------------------------ the copying walk's stores
// Every store of the copying walk goes through an address-space-1 pointer (global_store, counted by vmcnt
// only, like the loads of gptr) and is exactly as wide as the bytes that are due: a destination range abuts
// another lane's at byte granularity, so nothing is rounded up and nothing is read back.
__device__ __forceinline__ void stg_u8(uint8_t* p, uint32_t v) { *(EFES_GLOBAL uint8_t*)p = (uint8_t)v; }

typedef uint32_t wide_v4u __attribute__((ext_vector_type(4)));
typedef wide_v4u wide_v4u_u __attribute__((aligned(1)));  // a 16-byte piece at its destination: any alignment

// The 64 bytes of a block, as load_block_le left them, to d: four 16-byte stores at whatever alignment d has
// (store_piece of efes_crc_batch.hip).
__device__ __forceinline__ void store_block_le(uint8_t* d, const uint32_t (&le)[16]) {
  EFES_GLOBAL wide_v4u_u* o = (EFES_GLOBAL wide_v4u_u*)d;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const wide_v4u v = {le[4 * q], le[4 * q + 1], le[4 * q + 2], le[4 * q + 3]};
    o[q] = v;
  }
}

// wide_step for the copying walk: the block is first stored at d when `put` holds (the lane copies this
// member and the block is one of its own, not the dummy), then hashed, both from the same registers.
template <bool kSha, bool kCrc>
__device__ __forceinline__ void wide_step_put(const uint32_t (&le)[16], uint8_t* d, bool put, const WideCrcTab& t,
                                              uint32_t (&h)[5], uint32_t& crc_raw, bool live) {
  if (put) store_block_le(d, le);
  wide_step<kSha, kCrc>(le, t, h, crc_raw, live);
}

// wide_bulk (efes_wide_device.hpp) with every block also stored at d + 64 b when `cp` holds for the lane:
// the same loads in the same order -- the 128-byte-line pairing of the uniform phase, the unconditional
// loads with the dummy block of the ragged phase -- and a block's four stores issued in front of its
// rounds, from the buffer it is hashed from, so always before that buffer is reloaded.  A store issued
// after a prefetch never stands in front of it in the wave's one counter of outstanding memory operations;
// the stores that do stand in front of a prefetch are one and two blocks of rounds old when it is waited for.
// In the ragged phase a lane past its own last block holds the dummy and stores nothing.
template <bool kAligned16, bool kSha, bool kCrc>
__device__ __forceinline__ void wide_bulk_copy(const uint8_t* q, uint8_t* d, bool cp, uint64_t nbulk, uint64_t nmin,
                                               uint64_t nmax, const uint8_t* dummy, const WideCrcTab& t,
                                               uint32_t (&h)[5], uint32_t& crc_raw, uint32_t* prog, uint32_t w,
                                               uint32_t nw) {
  auto src = [&](uint64_t b) { return b < nbulk ? q + 64 * b : dummy; };
  uint32_t A[16], B[16], C[16];
  if (nmax == 0) return;
  load_block_le<kAligned16>(src(0), A);
  load_block_le<kAligned16>(src(1), B);
  uint64_t b = 0;
  for (; b + 5 < nmin; b += 4) {  // uniform phase: every lane has blocks b..b+5
    if (b % 32 == 0) wide_pace(prog, w, nw, (uint32_t)b);
    const uint8_t* qb = q + 64 * b;
    uint8_t* db = d + 64 * b;
    wide_step_put<kSha, kCrc>(A, db, cp, t, h, crc_raw, true);
    load_block_le<kAligned16>(qb + 128, A);
    load_block_le<kAligned16>(qb + 192, C);
    wide_step_put<kSha, kCrc>(B, db + 64, cp, t, h, crc_raw, true);
    wide_step_put<kSha, kCrc>(A, db + 128, cp, t, h, crc_raw, true);
    load_block_le<kAligned16>(qb + 256, A);
    load_block_le<kAligned16>(qb + 320, B);
    wide_step_put<kSha, kCrc>(C, db + 192, cp, t, h, crc_raw, true);
  }
  for (const uint64_t b_ragged = b; b < nmax; b += 3) {  // ragged phase: A, B hold blocks b, b+1 or the dummy
    if ((b - b_ragged) % 6 == 0) wide_pace(prog, w, nw, (uint32_t)b);
    uint8_t* db = d + 64 * b;
    load_block_le<kAligned16>(src(b + 2), C);
    wide_step_put<kSha, kCrc>(A, db, cp && b < nbulk, t, h, crc_raw, b < nbulk);
    if (b + 1 >= nmax) break;
    load_block_le<kAligned16>(src(b + 3), A);
    wide_step_put<kSha, kCrc>(B, db + 64, cp && b + 1 < nbulk, t, h, crc_raw, b + 1 < nbulk);
    if (b + 2 >= nmax) break;
    load_block_le<kAligned16>(src(b + 4), B);
    wide_step_put<kSha, kCrc>(C, db + 128, cp && b + 2 < nbulk, t, h, crc_raw, b + 2 < nbulk);
  }
}
template <bool kAligned16>
__device__ __forceinline__ void wide_bulk_copy_any(const uint8_t* q, uint8_t* d, bool cp, uint64_t nbulk,
                                                   uint64_t nmin, uint64_t nmax, const uint8_t* dummy, bool any_sha,
                                                   bool any_crc, const WideCrcTab& t, uint32_t (&h)[5],
                                                   uint32_t& crc_raw, uint32_t* prog, uint32_t w, uint32_t nw) {
  if (any_sha && any_crc) wide_bulk_copy<kAligned16, true, true>(q, d, cp, nbulk, nmin, nmax, dummy, t, h, crc_raw, prog, w, nw);
  else if (any_sha) wide_bulk_copy<kAligned16, true, false>(q, d, cp, nbulk, nmin, nmax, dummy, t, h, crc_raw, prog, w, nw);
  else if (any_crc) wide_bulk_copy<kAligned16, false, true>(q, d, cp, nbulk, nmin, nmax, dummy, t, h, crc_raw, prog, w, nw);
}

// ------------------------------------------------------------------ the walk's launch
// The persistent launch of a wide-walk kernel for njobs jobs: waves per SIMD as launch_wide, capped by what the
// kernel's registers and LDS admit on this device (asked of the runtime once per kernel and device).
template <auto kKernel, class... Args>
static hipError_t launch_wide_walk(uint32_t njobs, int cus, hipStream_t s, Args... args) {
  static std::mutex mu;
  static int8_t max_wps[64] = {};  // per device: 0 = not tried, -1 = failed, else the waves per SIMD that fit
  int dev = 0;
  (void)hipGetDevice(&dev);
  int cap;
  {
    std::lock_guard<std::mutex> lk(mu);
    int8_t& m = max_wps[dev & 63];
    if (m == 0) {
      m = -1;
      hipFuncAttributes fa{};
      if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kKernel)) == hipSuccess &&
          fa.sharedSizeBytes < kCuLds &&
          hipFuncSetAttribute(reinterpret_cast<const void*>(kKernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(kCuLds - fa.sharedSizeBytes)) == hipSuccess) {
        for (int w = kWideMaxWps; w >= 1 && m < 0; --w) {
          int per_cu = 0;
          const int block = 64 * kWideWaves * w;
          if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kKernel, block, (size_t)block * kXStride) ==
                  hipSuccess &&
              per_cu >= 1)
            m = (int8_t)w;
        }
      }
    }
    cap = m;
  }
  if (cap < 1) return hipErrorInvalidConfiguration;
  const uint64_t waves = ((uint64_t)njobs + 63) / 64, ncu = (uint64_t)(cus > 0 ? cus : 256);
  const uint32_t wps = (uint32_t)std::min<uint64_t>((uint64_t)cap, (waves + 4 * ncu - 1) / (4 * ncu));
  const uint32_t per = 64 * kWideWaves * wps;
  // Persistent grid: the workgroups that njobs chains would fill, or one per CU (a workgroup takes over
  // half of a CU's LDS at every wps).
  const uint64_t want = ((uint64_t)njobs + per - 1) / per;
  clear_last_error();
  hipLaunchKernelGGL(kKernel, dim3((uint32_t)std::min(want, ncu)), dim3(per), (size_t)per * kXStride, s, args...);
  return hipGetLastError();
}

}  // namespace efes
