// objects_results_invalid -- tables that break the rules of efes_hash.h "Object results", replayed against
// efes_objects_results_host on heap arrays of EXACT size.  Built with -fsanitize=address,undefined together with
// efes_amd/csrc/efes_objects.cpp (test_objects_results_host.py does that), so a read or write outside an array
// ends the program with a report; for every table the call must return EFES_OK, leave the words around its
// outputs alone and report verdicts of 0..3 whose counts add up.  Needs no GPU and no library.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "efes_hash.h"

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_seed ^= g_seed >> 12;
  g_seed ^= g_seed << 25;
  g_seed ^= g_seed >> 27;
  return (uint32_t)((g_seed * 0x2545F4914F6CDD1Dull) >> 32);
}

static const int32_t kStatuses[6] = {0, 0, 0, -2, -4, -99};
static int g_tables = 0;

#define REQUIRE(c)                                                        \
  do {                                                                    \
    if (!(c)) {                                                           \
      printf("FAILED %s:%d: %s (table %d)\n", __FILE__, __LINE__, #c, g_tables); \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

// One table: first[] as given (m + 1 words), n extents.  Every array is a heap block of exactly its size.
static void replay(const std::vector<uint32_t>& first_in, uint32_t n, bool with_expected, uint32_t compare) {
  const uint32_t m = (uint32_t)first_in.size() - 1;
  uint32_t* first = (uint32_t*)malloc(4 * (size_t)(m + 1));
  memcpy(first, first_in.data(), 4 * (size_t)(m + 1));
  int32_t* status = n ? (int32_t*)malloc(4 * (size_t)n) : nullptr;
  uint8_t* sums = n ? (uint8_t*)malloc(24 * (size_t)n) : nullptr;
  uint8_t* expected = with_expected && m ? (uint8_t*)malloc(24 * (size_t)m) : nullptr;
  for (uint32_t j = 0; j < n; ++j) status[j] = kStatuses[rnd() % 6];
  for (size_t k = 0; k < 24 * (size_t)n; ++k) sums[k] = (uint8_t)rnd();
  if (expected)
    for (size_t k = 0; k < 24 * (size_t)m; ++k) expected[k] = (uint8_t)rnd();
  efes_object_result* results = (efes_object_result*)malloc(sizeof(efes_object_result) * (size_t)(m ? m : 1));
  uint32_t* bad = (uint32_t*)malloc(4 * (size_t)(m ? m : 1));
  uint32_t* counts = (uint32_t*)malloc(16);
  memset(counts, 0xEE, 16);

  efes_objects in;
  memset(&in, 0, sizeof in);
  in.first = first;
  in.sums = sums;
  in.status = status;
  in.nobjects = m;
  in.nextents = n;
  efes_results req;
  memset(&req, 0, sizeof req);
  req.expected = expected;
  req.compare = compare;
  req.results = m ? results : nullptr;
  req.bad = m ? bad : nullptr;
  req.counts = counts;
  REQUIRE(efes_objects_results_host(&in, &req) == EFES_OK);
  uint32_t seen[4] = {0, 0, 0, 0};
  for (uint32_t i = 0; i < m; ++i) {
    REQUIRE(results[i].verdict <= EFES_VERDICT_EMPTY);
    ++seen[results[i].verdict];
  }
  for (int v = 0; v < 4; ++v) REQUIRE(counts[v] == seen[v]);
  const uint32_t nbad = counts[EFES_VERDICT_MISMATCH] + counts[EFES_VERDICT_FAILED];
  REQUIRE(nbad <= m);
  for (uint32_t k = 0; k < nbad; ++k) {
    REQUIRE(bad[k] < m && (k == 0 || bad[k - 1] < bad[k]));
    REQUIRE(results[bad[k]].verdict == EFES_VERDICT_MISMATCH || results[bad[k]].verdict == EFES_VERDICT_FAILED);
  }
  // the same with only the counters asked for
  uint32_t again[4];
  req.results = nullptr;
  req.bad = nullptr;
  req.counts = again;
  REQUIRE(efes_objects_results_host(&in, &req) == EFES_OK);
  REQUIRE(memcmp(again, counts, 16) == 0);
  free(first);
  free(status);
  free(sums);
  free(expected);
  free(results);
  free(bad);
  free(counts);
  ++g_tables;
}

static std::vector<uint32_t> well_formed(uint32_t m, uint32_t n) {
  std::vector<uint32_t> f(m + 1, 0);
  if (m == 0) return f;
  for (uint32_t i = 1; i < m; ++i) f[i] = rnd() % (n + 1);
  f[m] = n;
  for (uint32_t i = 1; i <= m; ++i)  // insertion sort: the tables are small
    for (uint32_t k = i; k > 0 && f[k - 1] > f[k]; --k) {
      const uint32_t t = f[k];
      f[k] = f[k - 1];
      f[k - 1] = t;
    }
  return f;
}

int main() {
  const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 257};
  for (uint32_t m : sizes)
    for (uint32_t n : sizes) {
      std::vector<uint32_t> good = well_formed(m, n);
      for (int expected = 0; expected < 2; ++expected) {
        replay(good, n, expected, 3);  // the well-formed table itself (with m == 0 < n: extents without an owner)
        std::vector<uint32_t> t(good.rbegin(), good.rend());  // decreasing
        replay(t, n, expected, 3);
        t = good;
        t[0] = 5;  // first[0] != 0
        replay(t, n, expected, 1);
        t = good;
        t[m] = n + 1000;  // first[nobjects] > nextents
        replay(t, n, expected, 2);
        t[m] = 0xFFFFFFFFu;
        replay(t, n, expected, 3);
        t = good;
        if (n > 3) t[m] = n - 3;  // the last extents have no owner behind them
        replay(t, n, expected, 3);
        t = good;
        t[m / 2] = 0xFFFFFFFFu;  // values near 2^32 in the middle
        if (m) t[m / 2 + (m / 2 < m ? 1 : 0)] = 0xFFFFFFFEu;
        replay(t, n, expected, 3);
        for (uint32_t& v : t) v = 0xFFFFFFFFu;
        replay(t, n, expected, 3);
        for (uint32_t& v : t) v = 0x80000000u + rnd() % 5;
        replay(t, n, expected, 3);
        for (uint32_t& v : t) v = rnd();  // anything at all
        replay(t, n, expected, 3);
        for (uint32_t& v : t) v = rnd() % (2 * n + 2);  // unordered, around the range
        replay(t, n, expected, 3);
      }
    }
  printf("%d tables ok\n", g_tables);
  return 0;
}
