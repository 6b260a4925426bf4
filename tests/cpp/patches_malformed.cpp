// patches_malformed -- efes_patches_table_host (efes_hash.h "PATCH logs") on heap arrays of EXACT size over logs of
// garbage: object indices anywhere in 32 bits, offsets and lengths anywhere in 64, nobjects from 1 upwards.  Built
// with -fsanitize=address,undefined together with efes_amd/csrc/efes_patches.cpp (test_patches_host.py does that), so
// a read or write outside an array ends the program with a report; asserted is the safety property: first[] is
// non-decreasing from 0 to npatches, patch_of is a permutation that agrees with answers[].slot, every slot lies in
// the segment of its clamped object, a refused slot is {0, 0}, the counters add up to npatches, and only the states
// of RESTARTED objects change.  Needs no GPU and no library.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "efes_hash.h"

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint64_t rnd64() {  // xorshift64*
  g_seed ^= g_seed >> 12;
  g_seed ^= g_seed << 25;
  g_seed ^= g_seed >> 27;
  return g_seed * 0x2545F4914F6CDD1Dull;
}
static uint32_t rnd() { return (uint32_t)(rnd64() >> 32); }

static int g_logs = 0;

#define REQUIRE(c)                                                                                   \
  do {                                                                                               \
    if (!(c)) {                                                                                      \
      printf("FAILED %s:%d: %s (m = %u, n = %u, variant %d)\n", __FILE__, __LINE__, #c, m, n, variant); \
      exit(1);                                                                                       \
    }                                                                                                \
  } while (0)

// One garbage field: small values, values around the powers of two and anything, so that offsets meet now and then.
static uint64_t garbage64() {
  switch (rnd() % 6) {
    case 0: return 0;
    case 1: return rnd() % 8;
    case 2: return ~0ull - rnd() % 4;
    case 3: return (1ull << (rnd() % 64)) - rnd() % 2;
    default: return rnd64();
  }
}

// variant bits: 1 = no offsets, 2 = no sha1, 4 = no crc32, 8 = no answers, 16 = no objects, 32 = no patch_of, 64 = no counts
static void replay(uint32_t m, uint32_t n, int variant) {
  efes_patch* log = n ? (efes_patch*)malloc(sizeof(efes_patch) * n) : nullptr;
  uint64_t* offsets = (uint64_t*)malloc(sizeof(uint64_t) * m);
  for (uint32_t i = 0; i < m; ++i) offsets[i] = garbage64();
  for (uint32_t a = 0; a < n; ++a) {
    log[a].data_offset = garbage64();
    log[a].length = garbage64();
    // a third of the PATCHes fit the upload's stored offset, so that chains form among the garbage
    const uint32_t object = rnd() % 4 ? rnd() % m : (rnd() % 2 ? rnd() : 0xFFFFFFFFu - rnd() % 2);
    log[a].object = object;
    log[a].file_offset = (rnd() % 3 == 0 && object < m) ? offsets[object] : garbage64();
    log[a].file_length = rnd() % 3 ? garbage64() : log[a].file_offset + log[a].length;
    log[a]._reserved = rnd();
  }
  efes_sha1_state* states = (efes_sha1_state*)malloc(sizeof(efes_sha1_state) * m);
  efes_sha1_state* states_before = (efes_sha1_state*)malloc(sizeof(efes_sha1_state) * m);
  efes_crc32_state* crcs = (efes_crc32_state*)malloc(sizeof(efes_crc32_state) * m);
  for (size_t k = 0; k < sizeof(efes_sha1_state) * m; ++k) ((unsigned char*)states)[k] = (unsigned char)(rnd() | 1u);
  memcpy(states_before, states, sizeof(efes_sha1_state) * m);
  efes_crc32_state* crcs_before = (efes_crc32_state*)malloc(sizeof(efes_crc32_state) * m);
  for (uint32_t i = 0; i < m; ++i) crcs_before[i].crc = crcs[i].crc = rnd() | 1u;
  efes_extent* extents = n ? (efes_extent*)malloc(sizeof(efes_extent) * n) : nullptr;
  uint32_t* first = (uint32_t*)malloc(sizeof(uint32_t) * ((size_t)m + 1));
  efes_patch_answer* answers = n ? (efes_patch_answer*)malloc(sizeof(efes_patch_answer) * n) : nullptr;
  efes_patch_object* objects = (efes_patch_object*)malloc(sizeof(efes_patch_object) * m);
  uint32_t* patch_of = n ? (uint32_t*)malloc(sizeof(uint32_t) * n) : nullptr;
  uint32_t* counts = (uint32_t*)malloc(sizeof(uint32_t) * 5);

  efes_patches p;
  memset(&p, 0, sizeof p);
  p.log = log;
  p.offsets = (variant & 1) ? nullptr : offsets;
  p.sha1 = (variant & 2) ? nullptr : states;
  p.crc32 = (variant & 4) ? nullptr : crcs;
  p.extents = extents;
  p.first = first;
  p.answers = (variant & 8) ? nullptr : answers;
  p.objects = (variant & 16) ? nullptr : objects;
  p.patch_of = (variant & 32) ? nullptr : patch_of;
  p.counts = (variant & 64) ? nullptr : counts;
  p.nobjects = m;
  p.npatches = n;
  REQUIRE(efes_patches_table_host(&p) == EFES_OK);

  REQUIRE(first[0] == 0 && first[m] == n);
  for (uint32_t i = 0; i < m; ++i) REQUIRE(first[i] <= first[i + 1]);
  if (p.patch_of) {
    bool* seen = (bool*)calloc(n ? n : 1, sizeof(bool));
    for (uint32_t k = 0; k < n; ++k) {
      REQUIRE(patch_of[k] < n && !seen[patch_of[k]]);
      seen[patch_of[k]] = true;
      const uint32_t object = log[patch_of[k]].object, i = object < m ? object : m - 1;
      REQUIRE(first[i] <= k && k < first[i + 1]);
      if (k && patch_of[k - 1] > patch_of[k]) REQUIRE(k == first[i]);  // arrival order inside a segment: the sort is stable
      if (p.answers) REQUIRE(answers[patch_of[k]].slot == k);
    }
    free(seen);
  }
  uint32_t tally[5] = {0, 0, 0, 0, 0};
  if (p.answers) {
    for (uint32_t a = 0; a < n; ++a) {
      const uint32_t v = answers[a].verdict, k = answers[a].slot;
      REQUIRE(v <= EFES_PATCH_INVALID && k < n);
      REQUIRE((v == EFES_PATCH_INVALID) == (log[a].object >= m));
      ++tally[v];
      if (v == EFES_PATCH_ADMITTED || v == EFES_PATCH_DONE)
        REQUIRE(extents[k].offset == log[a].data_offset && extents[k].length == log[a].length);
      else
        REQUIRE(extents[k].offset == 0 && extents[k].length == 0);
      if (v == EFES_PATCH_INVALID) REQUIRE(answers[a].offset == 0);
    }
    if (p.counts)
      for (int v = 0; v < 5; ++v) REQUIRE(counts[v] == tally[v]);
  }
  if (p.counts) REQUIRE((uint64_t)counts[0] + counts[1] + counts[2] + counts[3] + counts[4] == n);
  for (uint32_t i = 0; i < m; ++i) {
    const bool known = p.objects != nullptr;
    const bool restarted = known && (objects[i].flags & EFES_PATCH_OBJ_RESTARTED);
    if (known) {
      REQUIRE(!(objects[i].flags & ~7u) && objects[i].admitted <= first[i + 1] - first[i]);
      if (objects[i].admitted == 0) REQUIRE(objects[i].offset == (p.offsets ? offsets[i] : 0ull) && !restarted);
    }
    if (known && !restarted) {
      REQUIRE(memcmp(&states[i], &states_before[i], sizeof states[i]) == 0);
      REQUIRE(crcs[i].crc == crcs_before[i].crc);
    }
    if (restarted && p.sha1) {
      efes_sha1_state want;
      memset(&want, 0, sizeof want);
      want.h[0] = 0x67452301u, want.h[1] = 0xEFCDAB89u, want.h[2] = 0x98BADCFEu, want.h[3] = 0x10325476u, want.h[4] = 0xC3D2E1F0u;
      REQUIRE(memcmp(&states[i], &want, sizeof want) == 0);
    }
    if (restarted && p.crc32) REQUIRE(crcs[i].crc == 0);
    if (!p.sha1) REQUIRE(memcmp(&states[i], &states_before[i], sizeof states[i]) == 0);
    if (!p.crc32) REQUIRE(crcs[i].crc == crcs_before[i].crc);
  }
  ++g_logs;
  free(log);
  free(offsets);
  free(states);
  free(states_before);
  free(crcs);
  free(crcs_before);
  free(extents);
  free(first);
  free(answers);
  free(objects);
  free(patch_of);
  free(counts);
}

int main() {
  const uint32_t objects[] = {1, 2, 3, 64, 255, 256, 257, 1000};
  const uint32_t patches[] = {0, 1, 2, 63, 64, 65, 257, 1025, 4099};
  int variant = 0;
  for (uint32_t m : objects)
    for (uint32_t n : patches)
      for (int round = 0; round < 4; ++round) replay(m, n, round == 0 ? 0 : (variant = (variant * 37 + 11) & 127));
  replay(70000, 3000, 0);   // more objects than PATCHes
  replay(1, 100000, 0);     // one upload owns the whole log
  printf("%d logs ok\n", g_logs);
  return 0;
}
