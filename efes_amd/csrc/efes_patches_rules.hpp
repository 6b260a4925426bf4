// efes_patches_rules.hpp -- the rules of efes_patches_table (efes_hash.h "PATCH logs") that its device kernels
// (efes_patches.hip) and its host twin (efes_patches.cpp) share: the sort key of a PATCH, the step of the admission
// automaton (Go's saveFile, filereceiver.go:171-227, per object in arrival order), what a refused slot holds, the
// state a restarted upload begins from and the argument checks.  Plain inline functions, compiled for both sides,
// so the two sides cannot drift apart.
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

static_assert(sizeof(efes_patch) == 40 && sizeof(efes_patch_answer) == 16 && sizeof(efes_patch_object) == 16,
              "efes_patch / efes_patch_answer / efes_patch_object as efes_hash.h documents them");
constexpr uint32_t kPatchVerdicts = 5;  // words of efes_patches.counts
constexpr uint32_t kPatchClosedBits = EFES_PATCH_OBJ_DONE | EFES_PATCH_OBJ_DEFERRED;

// The sort key of a PATCH: its object, clamped into [0, nobjects); nobjects > 0.  An INVALID record lands in the
// last object's segment, where the automaton skips it.
EFES_HD uint32_t patch_key(uint32_t object, uint32_t nobjects) { return object < nobjects ? object : nobjects - 1; }

// Radix-256 digit passes that sort keys below nobjects: fixed on the host, so nothing is read back.
EFES_HD uint32_t patch_passes(uint32_t nobjects) { return nobjects <= 256u ? 1u : nobjects <= 65536u ? 2u : 3u; }

// One upload while its segment of the log is walked.  `closed` of the normative rules is flags & kPatchClosedBits
// (a DONE, or a restart behind admitted bytes, which is itself the first deferred PATCH); `acc` is admitted > 0.
struct PatchAuto {
  uint64_t cur;       // FileInfo.Offset
  uint32_t flags;     // EFES_PATCH_OBJ_*
  uint32_t admitted;  // PATCHes admitted so far
};

EFES_HD PatchAuto patch_begin(uint64_t offset) {
  PatchAuto a;
  a.cur = offset;
  a.flags = 0u;
  a.admitted = 0u;
  return a;
}

// One PATCH of the automaton's own object: the verdict, and in *answer the efes-file-offset header of the answer.
// Arithmetic is modulo 2^64, as Go's int64 addition is.
EFES_HD uint32_t patch_step(PatchAuto& a, uint64_t file_offset, uint64_t length, uint64_t file_length, uint64_t* answer) {
  *answer = a.cur;
  if (a.flags & kPatchClosedBits) {
    a.flags |= EFES_PATCH_OBJ_DEFERRED;
    return EFES_PATCH_DEFERRED;
  }
  if (file_offset == 0) {  // filereceiver.go:174-180: createFile + newFileInfo
    if (a.admitted) {      // one chain per object and table: the restart waits for the next log
      a.flags |= EFES_PATCH_OBJ_DEFERRED;
      return EFES_PATCH_DEFERRED;
    }
    a.flags |= EFES_PATCH_OBJ_RESTARTED;
    a.cur = length;
  } else if (file_offset == a.cur) {
    a.cur += length;
  } else {
    return EFES_PATCH_CONFLICT;  // :186-187, the required offset in *answer
  }
  ++a.admitted;
  *answer = a.cur;
  if (a.cur == file_length) {  // :219-224
    a.flags |= EFES_PATCH_OBJ_DONE;
    return EFES_PATCH_DONE;
  }
  return EFES_PATCH_ADMITTED;  // :226
}

EFES_HD bool patch_hashed(uint32_t verdict) { return verdict == EFES_PATCH_ADMITTED || verdict == EFES_PATCH_DONE; }

// NewSha1() (sha1.go:48-52) as the 26 32-bit words of an efes_sha1_state: h the five constants, x, _pad, nx and
// len zero.
EFES_HD uint32_t patch_fresh_word(uint32_t w) {
  return w == 0 ? 0x67452301u : w == 1 ? 0xEFCDAB89u : w == 2 ? 0x98BADCFEu : w == 3 ? 0x10325476u : w == 4 ? 0xC3D2E1F0u : 0u;
}
constexpr uint32_t kPatchStateWords = (uint32_t)(sizeof(efes_sha1_state) / 4);
static_assert(kPatchStateWords == 26, "an efes_sha1_state is 26 32-bit words");

// The argument checks that need no device and no scratch: EFES_OK or EFES_ERR_ARG.
inline int patches_check(const efes_patches* p) {
  if (!p || p->nobjects > EFES_OBJECTS_MAX || p->npatches > EFES_OBJECTS_MAX) return EFES_ERR_ARG;
  if (p->npatches && p->nobjects == 0) return EFES_ERR_ARG;
  if (!p->first) return EFES_ERR_ARG;  // first[nobjects] is always there
  if (p->npatches && (!p->log || !p->extents)) return EFES_ERR_ARG;
  if (((uintptr_t)p->log | (uintptr_t)p->offsets | (uintptr_t)p->sha1 | (uintptr_t)p->extents | (uintptr_t)p->answers |
       (uintptr_t)p->objects) & 7)
    return EFES_ERR_ARG;
  if (((uintptr_t)p->crc32 | (uintptr_t)p->first | (uintptr_t)p->patch_of | (uintptr_t)p->counts) & 3) return EFES_ERR_ARG;
  return EFES_OK;
}

}  // namespace efes
