// efes_infos.cpp -- efes_infos_unmarshal_text_host and efes_infos_marshal_text_host: the `.info` texts of an object
// table decoded into its states, and the states encoded back, on the HOST (efes_hash.h "Object infos").  The same
// rules as the device kernels (efes_infos_rules.hpp), one plain loop each; text may lie at any alignment, so every
// text word goes through memcpy.
#include <string.h>

#include "efes_infos_rules.hpp"

extern "C" int efes_infos_unmarshal_text_host(const efes_infos* in) {
  const int rc = efes::infos_check(in, false);
  if (rc != EFES_OK) return rc;
  uint32_t valid = 0;
  for (uint32_t i = 0; i < in->n; ++i) {
    const char* text = in->text + (size_t)EFES_INFO_TEXT_BYTES * i;
    uint32_t value[efes::kInfosTextWords];
    bool ok = true;  // all 208 characters count, whichever states are kept
    for (uint32_t w = 0; w < efes::kInfosTextWords; ++w) {
      uint64_t chars;
      memcpy(&chars, text + 8 * w, 8);
      ok &= efes::infos_decode_word(chars, &value[w]);
    }
    if (in->sha1) {
      uint32_t* s = reinterpret_cast<uint32_t*>(in->sha1 + i);
      for (uint32_t w = 0; w < efes::kInfosShaWords; ++w) {
        const uint32_t at = efes::infos_state_word(w);
        s[at] = ok ? efes::infos_word_value(w, value[w]) : efes::infos_refused_word(at);
      }
      s[efes::kInfosPadWord] = 0;
    }
    if (in->crc32) in->crc32[i].crc = ok ? value[efes::kInfosCrcWord] : 0u;
    if (in->status) in->status[i] = ok ? EFES_OK : EFES_ERR_INVALID_DIGEST;
    valid += ok ? 1u : 0u;
  }
  if (in->counts) {
    in->counts[0] = valid;
    in->counts[1] = in->n - valid;
  }
  return EFES_OK;
}

extern "C" int efes_infos_marshal_text_host(const efes_infos* in) {
  const int rc = efes::infos_check(in, false);
  if (rc != EFES_OK) return rc;
  for (uint32_t i = 0; i < in->n; ++i) {
    char* text = in->text + (size_t)EFES_INFO_TEXT_BYTES * i;
    const uint32_t* s = in->sha1 ? reinterpret_cast<const uint32_t*>(in->sha1 + i) : nullptr;
    for (uint32_t w = 0; w < efes::kInfosTextWords; ++w) {
      uint32_t v = 0;  // a digest the table does not keep marshals as zeros
      if (w == efes::kInfosCrcWord)
        v = in->crc32 ? in->crc32[i].crc : 0u;
      else if (s)
        v = efes::infos_word_value(w, s[efes::infos_state_word(w)]);
      const uint64_t chars = efes::infos_encode_word(v);
      memcpy(text + 8 * w, &chars, 8);
    }
  }
  return EFES_OK;
}
