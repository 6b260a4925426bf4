// efes_objects.cpp -- efes_objects_jobs_host: the object table expanded into job records on the HOST
// (efes_hash.h "Object tables").  The same rules as the device kernels (efes_objects_rules.hpp), one plain
// loop each; the base addresses in the table are only added to, never dereferenced.  Behind it
// efes_objects_results_host, the per-object results of such a table ("Object results"), likewise.
#include <string.h>

#include <vector>

#include "efes_objects_rules.hpp"

extern "C" int efes_objects_jobs_host(const efes_objects* in, const efes_objects_out* out) {
  const int rc = efes::objects_check(in, out);
  if (rc != EFES_OK) return rc;
  const uint32_t n = in->nextents, m = in->nobjects;
  const bool want_layout = out->layout != nullptr, want_dst = n && in->copy_to;
  if (!n && !want_layout) return EFES_OK;
  // E[j] = bytes in the extents before j; E[n] = all.  Without extents every size is 0 and first[] is not read.
  std::vector<uint64_t> E, L;
  try {
    E.resize((size_t)n + 1);
    if (!in->copy_offsets && (want_layout || want_dst)) L.resize((size_t)m + 1);
  } catch (...) {
    return EFES_ERR_NOMEM;
  }
  uint64_t at = 0;
  for (uint32_t j = 0; j < n; ++j) {
    E[j] = at;
    at += in->extents[j].length;
  }
  E[n] = at;
  auto size_of = [&](uint32_t i) -> uint64_t {
    return n ? E[efes::objects_bound(in->first, i + 1, n)] - E[efes::objects_bound(in->first, i, n)] : 0;
  };
  const uint64_t align = efes::objects_align_of(in);
  const uint64_t* layout = in->copy_offsets;
  if (!layout && (want_layout || want_dst)) {
    at = 0;
    for (uint32_t i = 0; i < m; ++i) {
      L[i] = at;
      at += efes::objects_round_up(size_of(i), align);
    }
    layout = L.data();
  }
  if (want_layout) {
    uint64_t room = 0;
    for (uint32_t i = 0; i < m; ++i) {
      out->layout[i] = layout[i];
      const uint64_t end = layout[i] + size_of(i);
      if (in->copy_offsets ? end > room : i + 1 == m) room = end;
    }
    out->layout[m] = room;
  }
  const uintptr_t data = (uintptr_t)in->data, sums = (uintptr_t)in->sums, copy_to = (uintptr_t)in->copy_to;
  for (uint32_t j = 0; j < n; ++j) {
    const uint32_t i = efes::objects_owner(in->first, m, j);
    efes_job& J = out->jobs[j];
    J.data = (const void*)(data + in->extents[j].offset);
    J.length = in->extents[j].length;
    J.sha1 = in->sha1 ? in->sha1 + i : nullptr;
    J.crc32 = in->crc32 ? in->crc32 + i : nullptr;
    J.sum = (uint8_t*)(sums + 24ull * j);
    J.status = in->status ? in->status + j : nullptr;
    J.flags = efes::objects_job_flags(in->first, m, i, j, in->flags);
    J._reserved = 0;
    if (in->ckpt) out->ckpt[j] = in->ckpt + j;
    if (want_dst) {
      const uint64_t here = m ? layout[i] : 0;
      out->dst[j] = (void*)(copy_to + here + (E[j] - E[efes::objects_bound(in->first, i, n)]));
    }
  }
  return EFES_OK;
}

// efes_objects_results_host: the per-object results (efes_hash.h "Object results") on the HOST.  The rules are
// results_object's, as on the device; the first failing member of every object is found as there, through the
// owner of each member that failed, so a table that breaks the rules gives the same in-range answers.
extern "C" int efes_objects_results_host(const efes_objects* in, const efes_results* req) {
  const int rc = efes::results_check(in, req);
  if (rc != EFES_OK) return rc;
  const uint32_t n = in->nextents, m = in->nobjects;
  std::vector<uint32_t> fail;
  try {
    fail.assign(m, efes::kResultsNone);
  } catch (...) {
    return EFES_ERR_NOMEM;
  }
  if (m)
    for (uint32_t j = 0; j < n; ++j) {
      if (in->status[j] == EFES_OK) continue;
      uint32_t& f = fail[efes::objects_owner(in->first, m, j)];
      if (j < f) f = j;
    }
  uint32_t counts[4] = {0, 0, 0, 0}, nbad = 0;
  for (uint32_t i = 0; i < m; ++i) {
    uint32_t w[efes::kResultWords];
    efes::results_object(in->first, n, in->status, in->sums, req->expected, req->compare, i, fail[i], w);
    if (req->results) memcpy(req->results + i, w, sizeof w);
    ++counts[w[7]];
    if (req->bad && efes::results_is_bad(w[7])) req->bad[nbad++] = i;
  }
  memcpy(req->counts, counts, sizeof counts);
  return EFES_OK;
}
