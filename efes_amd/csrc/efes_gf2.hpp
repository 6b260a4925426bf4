// efes_gf2.hpp -- GF(2) polynomial arithmetic mod the CRC-32/IEEE polynomial, shared by the span CRC
// (efes_crc_span.hip) and the batched CRC (efes_crc_batch.hip), host and device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace efes {

constexpr uint32_t kPolyReflected = 0xedb88320u;  // crc32.go:30 IEEE, reflected

// a * b mod P for polynomials in the reflected representation (bit 31 = x^0).  Branch-free, 32
// fixed steps (uniform control flow on the device).
__host__ __device__ inline uint32_t gf2_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - ((a >> (31 - i)) & 1u));
    b = (b >> 1) ^ (kPolyReflected & (0u - (b & 1u)));
  }
  return p;
}

// x^(8n) mod P: the operator that advances a raw CRC register over n zero bytes.
__host__ __device__ inline uint32_t xpow8n(uint64_t n) {
  uint32_t x2n[32];            // x^(2^k) mod P; x^(2^32) = x for this primitive P, so k cycles mod 32
  x2n[0] = 1u << 30;           // x^1
  for (int k = 1; k < 32; ++k) x2n[k] = gf2_mulmod(x2n[k - 1], x2n[k - 1]);
  uint32_t p = 1u << 31;       // x^0
  for (int k = 3; n; n >>= 1, ++k)
    if (n & 1) p = gf2_mulmod(x2n[k & 31], p);
  return p;
}

// The same from a ready table x2n[k] = x^(2^k) mod P (the device keeps one in memory: 31 squarings
// per call would cost more than the products).
__host__ __device__ inline uint32_t xpow8n(uint64_t n, const uint32_t* x2n) {
  uint32_t p = 1u << 31;
  for (int k = 3; n; n >>= 1, ++k)
    if (n & 1) p = gf2_mulmod(x2n[k & 31], p);
  return p;
}

}  // namespace efes
