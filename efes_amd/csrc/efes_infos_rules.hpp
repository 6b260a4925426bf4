// efes_infos_rules.hpp -- the rules of efes_infos_unmarshal_text and efes_infos_marshal_text (efes_hash.h "Object
// infos") that their device kernels (efes_infos.hip) and their host twins (efes_infos.cpp) share: which character is
// a hex digit, the map from a text position to a word of the state, the refusing image and the argument checks.
// Plain inline functions, compiled for both sides, so the two sides cannot drift apart.
//
// A record is 208 characters = 26 TEXT WORDS of 8 characters, each the hex of one big-endian 32-bit value
// (sha1_efes.go:26-34, crc32_efes.go:18-24).  efes_sha1_state is 26 STATE WORDS of 32 bits: h[0..4] (words 0-4), x
// (5-20), _pad (21), nx (22 low, 23 high), len (24 low, 25 high).  Text words 0-24 each fill one state word, text
// word 25 is the CRC, and _pad has no text.  Both sides are little-endian, as the state layouts already assume.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/efes_hash.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EFES_INFOS_HD __host__ __device__ inline
#else
#define EFES_INFOS_HD inline
#endif

namespace efes {

constexpr uint32_t kInfosTextWords = EFES_INFO_TEXT_BYTES / 8;  // 26: 25 of the SHA-1 state, then the CRC
constexpr uint32_t kInfosShaWords = 25;                         // text words that land in the SHA-1 state
constexpr uint32_t kInfosCrcWord = 25;                          // the text word of the CRC
constexpr uint32_t kInfosStateWords = (uint32_t)(sizeof(efes_sha1_state) / 4);  // 26, _pad included
constexpr uint32_t kInfosPadWord = 21;                                          // the state word no text word fills
constexpr uint32_t kInfosNxWord = 22;                                           // the low half of nx
static_assert(EFES_INFO_TEXT_BYTES == 208 && kInfosTextWords == 26 && kInfosStateWords == 26, "26 text words, 26 state words");
static_assert(sizeof(efes_infos) == 48, "efes_infos as efes_hash.h documents it");
static_assert(offsetof(efes_sha1_state, x) == 20 && offsetof(efes_sha1_state, _pad) == 4 * kInfosPadWord &&
                  offsetof(efes_sha1_state, nx) == 4 * kInfosNxWord && offsetof(efes_sha1_state, len) == 96 &&
                  sizeof(efes_crc32_state) == 4,
              "the word map below is that of efes_sha1_state");

// The value of a hex digit as Go's encoding/hex reads it (0-9, a-f, A-F), or 16 for every other byte.
EFES_INFOS_HD uint32_t infos_hex_value(uint32_t c) {
  if (c - (uint32_t)'0' < 10u) return c - (uint32_t)'0';
  const uint32_t lower = c | 0x20u;  // only 'A'-'F' and 'a'-'f' themselves land in 'a'-'f'
  if (lower - (uint32_t)'a' < 6u) return lower - (uint32_t)'a' + 10u;
  return 16u;
}

// Eight characters (the first in the lowest byte) as the big-endian 32-bit value they spell; false, and the value
// unspecified, when one of them is no hex digit.
EFES_INFOS_HD bool infos_decode_word(uint64_t chars, uint32_t* value) {
  uint32_t v = 0, bad = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t d = infos_hex_value((uint32_t)(chars >> (8 * k)) & 0xFFu);
    bad |= d;
    v = (v << 4) | (d & 15u);
  }
  *value = v;
  return (bad & 16u) == 0;
}

// The inverse: the eight lower-case characters of a big-endian 32-bit value, the first in the lowest byte.
EFES_INFOS_HD uint64_t infos_encode_word(uint32_t value) {
  uint64_t chars = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t d = (value >> (28 - 4 * k)) & 15u;
    chars |= (uint64_t)(d < 10u ? (uint32_t)'0' + d : (uint32_t)'a' + (d - 10u)) << (8 * k);
  }
  return chars;
}

// The state word that text word w < kInfosShaWords fills: h and x in place; nx and len are 64-bit big-endian in the
// text, so their high halves come first there and second in the state.
EFES_INFOS_HD uint32_t infos_state_word(uint32_t w) {
  if (w < 21u) return w;
  return w == 21u ? 23u : w == 22u ? 22u : w == 23u ? 25u : 24u;
}

// Between the big-endian value of text word w and the 32-bit word in memory: h, nx, len and the CRC are integers
// (the value itself); x lies as it is in the text, so its word is the value byte-swapped.  Its own inverse.
EFES_INFOS_HD uint32_t infos_word_value(uint32_t w, uint32_t v) {
  if (w < 5u || w >= 21u) return v;
  return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24);
}

// The refusing image: the state an invalid text leaves, every byte 0 except nx = EFES_SHA1_NX_REFUSED.
EFES_INFOS_HD uint32_t infos_refused_word(uint32_t state_word) { return state_word == kInfosNxWord ? (uint32_t)EFES_SHA1_NX_REFUSED : 0u; }

// The argument checks, which need no device: EFES_OK or EFES_ERR_ARG.  Only the device calls want text aligned.
inline int infos_check(const efes_infos* in, bool device) {
  if (!in || in->n > EFES_OBJECTS_MAX || in->_reserved) return EFES_ERR_ARG;
  if (in->n && (!in->text || (!in->sha1 && !in->crc32))) return EFES_ERR_ARG;
  if ((uintptr_t)in->sha1 & 7) return EFES_ERR_ARG;
  if (((uintptr_t)in->crc32 | (uintptr_t)in->status | (uintptr_t)in->counts) & 3) return EFES_ERR_ARG;
  if (device && ((uintptr_t)in->text & 7)) return EFES_ERR_ARG;
  return EFES_OK;
}

}  // namespace efes
