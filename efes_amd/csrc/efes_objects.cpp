// efes_objects.cpp -- efes_objects_jobs_host: the object table expanded into job records on the HOST
// (efes_hash.h "Object tables").  The same rules as the device kernels (efes_objects_rules.hpp), one plain
// loop each; the base addresses in the table are only added to, never dereferenced.  Behind it
// efes_objects_results_host, the per-object results of such a table ("Object results"), likewise; and
// efes_objects_order_host and efes_objects_jobs_ordered_host ("Object order"), the ranking and the ordered build.
#include <string.h>

#include <algorithm>
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

// efes_objects_order_host: the longest-first ranking (efes_hash.h "Object order") on the HOST: the keys of
// order_key over the sizes of order_size, as on the device, and a stable sort from the identity.
extern "C" int efes_objects_order_host(const efes_objects* in, uint32_t* order) {
  const int rc = efes::order_check(in, order);
  if (rc != EFES_OK) return rc;
  const uint32_t n = in->nextents, m = in->nobjects;
  if (m == 0) return EFES_OK;
  std::vector<uint64_t> E, key;
  std::vector<uint32_t> idx;
  try {
    E.resize((size_t)n + 1);
    key.resize(m);
    idx.resize(m);
  } catch (...) {
    return EFES_ERR_NOMEM;
  }
  uint64_t at = 0;
  for (uint32_t j = 0; j < n; ++j) {
    E[j] = at;
    at += in->extents[j].length;
  }
  E[n] = at;
  for (uint32_t i = 0; i < m; ++i) {
    key[i] = efes::order_key(efes::order_size(in->first, E.data(), i, n));
    idx[i] = i;
  }
  try {
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
  } catch (...) {  // its temporary buffer
    return EFES_ERR_NOMEM;
  }
  memcpy(order, idx.data(), (size_t)m * sizeof(uint32_t));
  return EFES_OK;
}

// efes_objects_jobs_ordered_host: efes_objects_jobs_host with the objects emitted in the order given.  The layout
// is the table's, as there; every slot goes through order_slot, order_job_words and order_job_dst, as on the device.
extern "C" int efes_objects_jobs_ordered_host(const efes_objects* in, const efes_objects_out* out, const uint32_t* order,
                                              uint32_t* job_first) {
  const int rc = efes::ordered_check(in, out, order, job_first);
  if (rc != EFES_OK) return rc;
  const uint32_t n = in->nextents, m = in->nobjects;
  const bool want_layout = out->layout != nullptr, want_dst = n && in->copy_to;
  if (!n && !want_layout && !job_first) return EFES_OK;
  std::vector<uint64_t> E, L, J;
  try {
    E.resize((size_t)n + 1);
    J.resize((size_t)m + 1);
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
  const uint64_t align = efes::objects_align_of(in);
  const uint64_t* layout = in->copy_offsets;
  if (!layout && (want_layout || want_dst)) {
    at = 0;
    for (uint32_t i = 0; i < m; ++i) {
      L[i] = at;
      at += efes::objects_round_up(efes::order_size(in->first, E.data(), i, n), align);
    }
    layout = L.data();
  }
  if (want_layout) {
    uint64_t room = 0;
    for (uint32_t i = 0; i < m; ++i) {
      out->layout[i] = layout[i];
      const uint64_t end = layout[i] + efes::order_size(in->first, E.data(), i, n);
      if (in->copy_offsets ? end > room : i + 1 == m) room = end;
    }
    out->layout[m] = room;
  }
  at = 0;  // without extents every count is 0 and neither first[] nor order[] is read
  for (uint32_t r = 0; r < m; ++r) {
    J[r] = at;
    if (n) at += efes::order_count(in->first, efes::order_object(order, m, r), n);
  }
  J[m] = at;
  if (job_first)
    for (uint32_t r = 0; r <= m; ++r) job_first[r] = efes::order_job_first(J[r], n);
  for (uint32_t k = 0; k < n; ++k) {
    const efes::OrderSlot s = efes::order_slot(in->first, order, J.data(), m, n, k);
    uint64_t w[efes::kJobWords];
    efes::order_job_words(*in, s.i, s.j, w);
    memcpy(static_cast<void*>(out->jobs + k), w, sizeof w);
    if (in->ckpt) out->ckpt[k] = in->ckpt + s.j;
    if (want_dst) out->dst[k] = (void*)(uintptr_t)efes::order_job_dst(*in, E.data(), layout, s.i, s.j);
  }
  return EFES_OK;
}
