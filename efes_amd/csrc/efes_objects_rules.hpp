// efes_objects_rules.hpp -- the rules of efes_objects_jobs (efes_hash.h) that its device kernels
// (efes_objects.hip) and its host twin (efes_objects.cpp) share: the owner of an extent, the flag word of
// its job, the rounding of the default layout and the argument checks; and the rules of efes_objects_results
// that efes_objects_results.hip and its host twin share: the status pick, the sum pick, the verdict and the
// argument checks; and the rules of efes_objects_order and efes_objects_jobs_ordered that efes_objects_order.hip and
// their host twins share: the sort key, the slot -> (rank, object, extent) mapping, the job words and the argument
// checks.  Plain inline functions, compiled for both sides, so the two sides cannot drift apart.
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

// ---- object order (efes_objects_order, efes_objects_jobs_ordered and their host twins)
// E is the exclusive scan of the extents' lengths, E[0, nextents]; J the exclusive scan of the extent counts in
// rank order, J[0, nobjects].

// Bytes of object i < nobjects, modulo 2^64, both boundaries clamped into E[0, nextents]; 0 without extents
// (E is then not read).
EFES_HD uint64_t order_size(const uint32_t* first, const uint64_t* E, uint32_t i, uint32_t nextents) {
  return nextents ? E[objects_bound(first, i + 1, nextents)] - E[objects_bound(first, i, nextents)] : 0ull;
}

// The sort key of a size: ascending keys are descending sizes, so a stable ascending sort from the identity is
// "longest first, equal sizes in ascending table index".
EFES_HD uint64_t order_key(uint64_t size) { return ~size; }

// Digit d (0 = least significant byte) of a key; the sort's radix is 256.
EFES_HD uint32_t order_digit(uint64_t key, uint32_t d) { return (uint32_t)(key >> (8u * d)) & 0xFFu; }

// Extents of object i < nobjects: the distance of its clamped boundaries, 0 where the table decreases.
EFES_HD uint32_t order_count(const uint32_t* first, uint32_t i, uint32_t nextents) {
  const uint32_t b = objects_bound(first, i, nextents), e = objects_bound(first, i + 1, nextents);
  return e > b ? e - b : 0u;
}

// order[r] clamped into [0, nobjects); nobjects > 0.
EFES_HD uint32_t order_object(const uint32_t* order, uint32_t nobjects, uint32_t r) {
  const uint32_t i = order[r];
  return i < nobjects ? i : nobjects - 1;
}

// The largest r in [0, nobjects) with J[r] <= k, or 0 if there is none: objects_owner over the 64-bit J.
EFES_HD uint32_t order_rank(const uint64_t* J, uint32_t nobjects, uint32_t k) {
  uint32_t lo = 0, hi = nobjects;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (J[mid] <= (uint64_t)k)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo ? lo - 1 : 0;
}

// Slot k < nextents of the ordered job array: its rank r, its object i = order[r] and its extent j, every one an
// index of its range whatever first[], order[] and so J[] hold.  With nobjects == 0 the one index there is, 0, is
// used, as efes_objects_jobs does (order and J are then not read).
struct OrderSlot {
  uint32_t r, i, j;
};
EFES_HD OrderSlot order_slot(const uint32_t* first, const uint32_t* order, const uint64_t* J, uint32_t nobjects,
                             uint32_t nextents, uint32_t k) {
  OrderSlot s;
  if (nobjects == 0) {
    s.r = 0;
    s.i = 0;
    s.j = k;
    return s;
  }
  s.r = order_rank(J, nobjects, k);
  s.i = order_object(order, nobjects, s.r);
  const uint64_t at = J[s.r] <= (uint64_t)k ? (uint64_t)k - J[s.r] : 0ull;  // J[0] == 0, so only a broken J is above k
  const uint64_t j = (uint64_t)objects_bound(first, s.i, nextents) + at;
  s.j = j < (uint64_t)nextents ? (uint32_t)j : nextents - 1;
  return s;
}

// The seven 64-bit words of the job of extent j of object i: what efes_objects_jobs writes at jobs[j] where
// i = owner(j).  j < nextents; i < max(nobjects, 1).
EFES_HD void order_job_words(const efes_objects& in, uint32_t i, uint32_t j, uint64_t w[kJobWords]) {
  const efes_extent e = in.extents[j];
  w[0] = (uint64_t)(uintptr_t)in.data + e.offset;
  w[1] = e.length;
  w[2] = in.sha1 ? (uint64_t)(uintptr_t)(in.sha1 + i) : 0ull;
  w[3] = in.crc32 ? (uint64_t)(uintptr_t)(in.crc32 + i) : 0ull;
  w[4] = (uint64_t)(uintptr_t)in.sums + 24ull * j;
  w[5] = in.status ? (uint64_t)(uintptr_t)(in.status + j) : 0ull;
  w[6] = (uint64_t)objects_job_flags(in.first, in.nobjects, i, j, in.flags);  // _reserved = 0 in the upper half
}

// The destination of extent j of object i: copy_to + L[i] + the bytes of the object's extents before j.
EFES_HD uint64_t order_job_dst(const efes_objects& in, const uint64_t* E, const uint64_t* L, uint32_t i, uint32_t j) {
  const uint64_t at = in.nobjects && L ? L[i] : 0ull;
  return (uint64_t)(uintptr_t)in.copy_to + at + (E[j] - E[objects_bound(in.first, i, in.nextents)]);
}

// job_first[r] of a J[r]: saturated at nextents.
EFES_HD uint32_t order_job_first(uint64_t Jr, uint32_t nextents) { return Jr < (uint64_t)nextents ? (uint32_t)Jr : nextents; }

// The argument checks of efes_objects_order that need no device and no scratch: EFES_OK or EFES_ERR_ARG.
inline int order_check(const efes_objects* in, const uint32_t* order) {
  if (!in || in->nobjects > EFES_OBJECTS_MAX || in->nextents > EFES_OBJECTS_MAX) return EFES_ERR_ARG;
  if (in->nextents && !in->extents) return EFES_ERR_ARG;
  if (in->nobjects == 0) return EFES_OK;
  if (!in->first || !order || ((uintptr_t)order & 3)) return EFES_ERR_ARG;
  return EFES_OK;
}

// Those of efes_objects_jobs_ordered: the builder's, and an order for a table that has objects; order and job_first
// are arrays of 32-bit words.
inline int ordered_check(const efes_objects* in, const efes_objects_out* out, const uint32_t* order, const uint32_t* job_first) {
  const int rc = objects_check(in, out);
  if (rc != EFES_OK) return rc;
  if (in->nobjects && !order) return EFES_ERR_ARG;
  if (((uintptr_t)order | (uintptr_t)job_first) & 3) return EFES_ERR_ARG;
  return EFES_OK;
}

}  // namespace efes
