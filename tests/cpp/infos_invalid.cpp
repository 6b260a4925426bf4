// infos_invalid -- efes_infos_unmarshal_text_host and efes_infos_marshal_text_host (efes_hash.h "Object infos") on
// heap arrays of EXACT size, with text at an odd address and the first and last records spoiled.  Built with
// -fsanitize=address,undefined together with efes_amd/csrc/efes_infos.cpp (test_infos_host.py does that), so a read
// or write outside an array ends the program with a report; the round trip states -> texts -> states must give the
// states back (with _pad 0), and a spoiled record the refusing image.  Needs no GPU and no library.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "efes_hash.h"

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {  // xorshift64*
  g_seed ^= g_seed >> 12;
  g_seed ^= g_seed << 25;
  g_seed ^= g_seed >> 27;
  return (uint32_t)((g_seed * 0x2545F4914F6CDD1Dull) >> 32);
}

static int g_records = 0;

#define REQUIRE(c)                                                                  \
  do {                                                                              \
    if (!(c)) {                                                                     \
      printf("FAILED %s:%d: %s (n = %u, variant %d)\n", __FILE__, __LINE__, #c, n, variant); \
      exit(1);                                                                      \
    }                                                                               \
  } while (0)

static const size_t kPositions[] = {0, 7, 8, 39, 40, 167, 168, 183, 184, 199, 200, 207};
static const unsigned char kBytes[] = {'g', 'G', '/', ':', '@', '`', ' ', 0x00, 0x80, 0xFF};

// variant bits: 1 = no sha1, 2 = no crc32, 4 = no status, 8 = no counts
static void replay(uint32_t n, int variant) {
  const bool with_sha = !(variant & 1), with_crc = !(variant & 2), with_status = !(variant & 4), with_counts = !(variant & 8);
  efes_sha1_state* states = n ? (efes_sha1_state*)malloc(sizeof(efes_sha1_state) * n) : nullptr;
  efes_crc32_state* crcs = n ? (efes_crc32_state*)malloc(sizeof(efes_crc32_state) * n) : nullptr;
  for (size_t k = 0; k < sizeof(efes_sha1_state) * n; ++k) ((unsigned char*)states)[k] = (unsigned char)rnd();
  for (uint32_t i = 0; i < n; ++i) crcs[i].crc = rnd();
  // the text one byte into a block of 208 n + 1: an odd address, and not one byte to spare behind it
  char* block = (char*)malloc((size_t)EFES_INFO_TEXT_BYTES * n + 1);
  char* text = block + 1;

  efes_infos m;
  memset(&m, 0, sizeof m);
  m.text = n ? text : nullptr;
  m.sha1 = with_sha ? states : nullptr;
  m.crc32 = with_crc ? crcs : nullptr;
  m.n = n;
  REQUIRE(efes_infos_marshal_text_host(&m) == EFES_OK);
  for (size_t k = 0; k < (size_t)EFES_INFO_TEXT_BYTES * n; ++k)
    REQUIRE((text[k] >= '0' && text[k] <= '9') || (text[k] >= 'a' && text[k] <= 'f'));

  // spoil the first and the last record, and one in the middle where there is one
  bool* bad = (bool*)calloc(n ? n : 1, sizeof(bool));
  const uint32_t chosen[3] = {0, n ? n - 1 : 0, n / 2};
  for (int c = 0; c < 3 && n; ++c) {
    const uint32_t i = chosen[c];
    text[(size_t)EFES_INFO_TEXT_BYTES * i + kPositions[rnd() % 12]] = (char)kBytes[rnd() % 10];
    bad[i] = true;
  }

  efes_sha1_state* out_states = n ? (efes_sha1_state*)malloc(sizeof(efes_sha1_state) * n) : nullptr;
  efes_crc32_state* out_crcs = n ? (efes_crc32_state*)malloc(sizeof(efes_crc32_state) * n) : nullptr;
  int32_t* status = n ? (int32_t*)malloc(sizeof(int32_t) * n) : nullptr;
  uint32_t* counts = (uint32_t*)malloc(2 * sizeof(uint32_t));
  counts[0] = counts[1] = 0xEEEEEEEEu;
  efes_infos u;
  memset(&u, 0, sizeof u);
  u.text = n ? text : nullptr;
  u.sha1 = with_sha ? out_states : nullptr;
  u.crc32 = with_crc ? out_crcs : nullptr;
  u.status = with_status ? status : nullptr;
  u.counts = with_counts ? counts : nullptr;
  u.n = n;
  REQUIRE(efes_infos_unmarshal_text_host(&u) == EFES_OK);
  uint32_t nbad = 0;
  for (uint32_t i = 0; i < n; ++i) {
    nbad += bad[i] ? 1u : 0u;
    if (with_status) REQUIRE(status[i] == (bad[i] ? EFES_ERR_INVALID_DIGEST : EFES_OK));
    if (with_crc) REQUIRE(out_crcs[i].crc == (bad[i] ? 0u : crcs[i].crc));
    if (!with_sha) continue;
    efes_sha1_state want;
    if (bad[i]) {
      memset(&want, 0, sizeof want);
      want.nx = EFES_SHA1_NX_REFUSED;
    } else {
      want = states[i];
      want._pad = 0;
    }
    REQUIRE(memcmp(&out_states[i], &want, sizeof want) == 0);
  }
  if (with_counts) REQUIRE(counts[0] == n - nbad && counts[1] == nbad);
  g_records += (int)n;
  free(states);
  free(crcs);
  free(block);
  free(bad);
  free(out_states);
  free(out_crcs);
  free(status);
  free(counts);
}

int main() {
  const uint32_t sizes[] = {0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 257, 1025};
  for (uint32_t n : sizes)
    for (int variant = 0; variant < 16; ++variant)
      if ((variant & 3) != 3) replay(n, variant);  // sha1 and crc32 are not both NULL
  printf("%d records ok\n", g_records);
  return 0;
}
