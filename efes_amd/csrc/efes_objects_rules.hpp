// efes_objects_rules.hpp -- the rules of efes_objects_jobs (efes_hash.h) that its device kernels
// (efes_objects.hip) and its host twin (efes_objects.cpp) share: the owner of an extent, the flag word of
// its job, the rounding of the default layout and the argument checks; and the rules of efes_objects_results
// that efes_objects_results.hip and its host twin share: the status pick, the sum pick, the verdict and the
// argument checks.  Plain inline functions, compiled for both sides, so the two sides cannot drift apart.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/efes_hash.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EFES_HD __host__ __device__ inline
#else
#define EFES_HD inline
#endif

namespace efes {

constexpr uint32_t kObjectsFlagBits = EFES_OBJECTS_FRESH | EFES_OBJECTS_RUNNING;
constexpr uint32_t kObjectsMaxAlign = 1u << 20;
constexpr int kJobWords = (int)(sizeof(efes_job) / 8);  // 64-bit words of one job record
static_assert(sizeof(efes_job) == 56 && kJobWords == 7, "a job is seven 64-bit words");
static_assert(sizeof(efes_extent) == 16 && sizeof(efes_objects) == 96 && sizeof(efes_objects_out) == 32,
              "efes_extent / efes_objects / efes_objects_out as efes_hash.h documents them");

// The largest i in [0, nobjects) with first[i] <= j, or 0 if there is none (nobjects == 0 included): a
// binary search over first[0, nobjects) that reads no other word and returns an index inside
// [0, max(nobjects, 1)) whatever first[] holds.  This clamp is the call's safety property.
EFES_HD uint32_t objects_owner(const uint32_t* first, uint32_t nobjects, uint32_t j) {
  uint32_t lo = 0, hi = nobjects;  // first[i] <= j for the i < lo that were looked at, > j for those >= hi
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= j)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo ? lo - 1 : 0;
}

// first[k] clamped to an index of E[0, nextents]; k <= nobjects.
EFES_HD uint32_t objects_bound(const uint32_t* first, uint32_t k, uint32_t nextents) {
  const uint32_t f = first[k];
  return f < nextents ? f : nextents;
}

// The flag word of extent j of object i = objects_owner(j): INIT (FRESH) or nothing on the object's first
// extent, CHAIN on every other, FINALIZE on its last or (RUNNING) on all.  first[i + 1] is read only where
// the table has it (i + 1 <= nobjects).
EFES_HD uint32_t objects_job_flags(const uint32_t* first, uint32_t nobjects, uint32_t i, uint32_t j, uint32_t flags) {
  uint32_t f = first[i] == j ? ((flags & EFES_OBJECTS_FRESH) ? EFES_JOB_INIT : 0u) : EFES_JOB_CHAIN;
  const bool last = i < nobjects && first[i + 1] == j + 1u;
  if (last || (flags & EFES_OBJECTS_RUNNING)) f |= EFES_JOB_FINALIZE;
  return f;
}

EFES_HD uint64_t objects_round_up(uint64_t size, uint64_t align) { return (size + (align - 1)) & ~(align - 1); }

EFES_HD uint32_t objects_align_of(const efes_objects* in) { return in->copy_align ? in->copy_align : EFES_OBJECTS_COPY_ALIGN; }

// The argument checks that need no device and no scratch: EFES_OK or EFES_ERR_ARG.
inline int objects_check(const efes_objects* in, const efes_objects_out* out) {
  if (!in || !out || in->nobjects > EFES_OBJECTS_MAX || in->nextents > EFES_OBJECTS_MAX) return EFES_ERR_ARG;
  if (in->nextents == 0) return EFES_OK;
  if (!in->extents || !in->first || !in->sums || !out->jobs) return EFES_ERR_ARG;
  if (!in->sha1 && !in->crc32) return EFES_ERR_ARG;
  if ((in->copy_to && !out->dst) || (in->ckpt && !out->ckpt)) return EFES_ERR_ARG;
  if (in->copy_offsets && !in->copy_to) return EFES_ERR_ARG;
  if (in->flags & ~kObjectsFlagBits) return EFES_ERR_ARG;
  const uint32_t a = in->copy_align;
  if (a && ((a & (a - 1)) || a > kObjectsMaxAlign)) return EFES_ERR_ARG;
  return EFES_OK;
}

// ---- object results (efes_objects_results, efes_objects_results_host)
static_assert(sizeof(efes_object_result) == 32 && sizeof(efes_results) == 40,
              "efes_object_result / efes_results as efes_hash.h documents them");
constexpr uint32_t kResultsCompareBits = EFES_HASH_SHA1 | EFES_HASH_CRC32;
constexpr uint32_t kResultsNone = 0xFFFFFFFFu;  // the per-object "first failing member" word: no member failed
constexpr int kResultWords = (int)(sizeof(efes_object_result) / 4);

// The word of sums or expected at 32-bit index w (both are 4-byte aligned: results_check).
EFES_HD uint32_t results_word(const uint8_t* bytes, size_t w) { return reinterpret_cast<const uint32_t*>(bytes)[w]; }

// The eight 32-bit words of object i's result: the sum as six words in memory order, the status, the verdict.
// fail is the lowest index of a member of i whose status is not EFES_OK, or kResultsNone.  Reads first[i] and
// first[i + 1], clamped into [0, nextents]; at most two statuses (the one fail names and, where that is another
// member, the last one's), each at an index below nextents; at most one sum and, for an object all of whose
// members are EFES_OK, one expected entry.
EFES_HD void results_object(const uint32_t* first, uint32_t nextents, const int32_t* status, const uint8_t* sums,
                            const uint8_t* expected, uint32_t compare, uint32_t i, uint32_t fail, uint32_t out[kResultWords]) {
#pragma unroll
  for (int k = 0; k < kResultWords; ++k) out[k] = 0u;
  const uint32_t begin = objects_bound(first, i, nextents), end = objects_bound(first, i + 1, nextents);
  if (end <= begin) {  // no extents (or a table that decreases here)
    out[7] = EFES_VERDICT_EMPTY;
    return;
  }
  const uint32_t l = end - 1;  // < nextents
  int32_t st = EFES_OK;
  bool last_ok = true;
  if (fail != kResultsNone) {
    const uint32_t f = fail < nextents ? fail : l;  // the atomic minimum only ever holds an extent index
    st = status[f];
    last_ok = f != l && status[l] == EFES_OK;
  }
  if (last_ok) {
#pragma unroll
    for (int k = 0; k < 6; ++k) out[k] = results_word(sums, 6 * (size_t)l + k);
  }
  out[6] = (uint32_t)st;
  if (st != EFES_OK) {
    out[7] = EFES_VERDICT_FAILED;
    return;
  }
  uint32_t diff = 0;
  if (expected && compare) {
    const uint32_t sha = (compare & EFES_HASH_SHA1) ? 0xFFFFFFFFu : 0u, crc = (compare & EFES_HASH_CRC32) ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) diff |= (out[k] ^ results_word(expected, 6 * (size_t)i + k)) & (k < 5 ? sha : crc);
  }
  out[7] = diff ? EFES_VERDICT_MISMATCH : EFES_VERDICT_OK;
}

EFES_HD bool results_is_bad(uint32_t verdict) { return verdict == EFES_VERDICT_MISMATCH || verdict == EFES_VERDICT_FAILED; }

// The argument checks that need no device and no scratch: EFES_OK or EFES_ERR_ARG.
inline int results_check(const efes_objects* in, const efes_results* req) {
  if (!in || !req || !req->counts) return EFES_ERR_ARG;
  if (in->nobjects > EFES_OBJECTS_MAX || in->nextents > EFES_OBJECTS_MAX) return EFES_ERR_ARG;
  if ((req->compare & ~kResultsCompareBits) || req->_reserved) return EFES_ERR_ARG;
  if (in->nobjects && !in->first) return EFES_ERR_ARG;
  if (in->nextents && (!in->sums || !in->status)) return EFES_ERR_ARG;
  if (((uintptr_t)in->sums | (uintptr_t)req->expected | (uintptr_t)req->bad | (uintptr_t)req->counts) & 3) return EFES_ERR_ARG;
  if ((uintptr_t)req->results & 7) return EFES_ERR_ARG;
  return EFES_OK;
}

}  // namespace efes
