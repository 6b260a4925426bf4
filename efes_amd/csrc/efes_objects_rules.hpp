// efes_objects_rules.hpp -- the rules of efes_objects_jobs (efes_hash.h) that its device kernels
// (efes_objects.hip) and its host twin (efes_objects.cpp) share: the owner of an extent, the flag word of
// its job, the rounding of the default layout and the argument checks.  Plain inline functions, compiled
// for both sides, so the two builders cannot drift apart.
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

}  // namespace efes
