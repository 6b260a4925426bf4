// efes_patches.cpp -- efes_patches_table_host: the object table of an arrival log of PATCH requests, made on the
// HOST (efes_hash.h "PATCH logs").  The same rules as the device kernels (efes_patches_rules.hpp): a counting sort
// by the clamped object gives first[] and every PATCH's slot, then the automaton runs over the log in arrival order,
// which is each object's segment order because the sort is stable.
#include <stdlib.h>
#include <string.h>

#include "efes_patches_rules.hpp"

extern "C" int efes_patches_table_host(const efes_patches* in) {
  const int rc = efes::patches_check(in);
  if (rc != EFES_OK) return rc;
  const uint32_t m = in->nobjects, n = in->npatches;
  efes::PatchAuto* autos = nullptr;
  uint32_t* next = nullptr;  // the next free slot of every object
  if (m) {
    autos = static_cast<efes::PatchAuto*>(malloc(sizeof(efes::PatchAuto) * m));
    next = static_cast<uint32_t*>(calloc(m, sizeof(uint32_t)));
    if (!autos || !next) {
      free(autos);
      free(next);
      return EFES_ERR_NOMEM;
    }
  }
  uint32_t counts[efes::kPatchVerdicts] = {0, 0, 0, 0, 0};
  for (uint32_t a = 0; a < n; ++a) ++next[efes::patch_key(in->log[a].object, m)];
  uint32_t at = 0;
  for (uint32_t i = 0; i < m; ++i) {
    const uint32_t c = next[i];
    in->first[i] = next[i] = at;
    at += c;
    autos[i] = efes::patch_begin(in->offsets ? in->offsets[i] : 0ull);
  }
  in->first[m] = n;
  for (uint32_t a = 0; a < n; ++a) {
    const efes_patch p = in->log[a];
    const uint32_t i = efes::patch_key(p.object, m), k = next[i]++;
    uint64_t answer = 0;
    const uint32_t verdict =
        p.object < m ? efes::patch_step(autos[i], p.file_offset, p.length, p.file_length, &answer) : EFES_PATCH_INVALID;
    const bool hashed = efes::patch_hashed(verdict);
    in->extents[k].offset = hashed ? p.data_offset : 0ull;
    in->extents[k].length = hashed ? p.length : 0ull;
    if (in->answers) {
      in->answers[a].offset = answer;
      in->answers[a].verdict = verdict;
      in->answers[a].slot = k;
    }
    if (in->patch_of) in->patch_of[k] = a;
    ++counts[verdict];
  }
  for (uint32_t i = 0; i < m; ++i) {
    if (in->objects) {
      in->objects[i].offset = autos[i].cur;
      in->objects[i].flags = autos[i].flags;
      in->objects[i].admitted = autos[i].admitted;
    }
    if (!(autos[i].flags & EFES_PATCH_OBJ_RESTARTED)) continue;
    if (in->sha1) {
      uint32_t* s = reinterpret_cast<uint32_t*>(in->sha1 + i);
      for (uint32_t w = 0; w < efes::kPatchStateWords; ++w) s[w] = efes::patch_fresh_word(w);
    }
    if (in->crc32) in->crc32[i].crc = 0u;
  }
  if (in->counts) memcpy(in->counts, counts, sizeof counts);
  free(autos);
  free(next);
  return EFES_OK;
}
