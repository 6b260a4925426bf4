// gathercopy.hip -- a plain single-launch gather of byte-granular device extents (measurement infrastructure for
// tools/bench_hash_chain_copy.py, not part of libefeshash): the copy a caller issues today behind
// efes_hash_chain_wide when the extents have unequal lengths and no strided view describes them.
//
// Extent j is len[j] bytes from src[j] to dst[j], any alignment on either side.  The extents are cut into chunks
// of 16 KiB; chunk c belongs to the extent j with first[j] <= c < first[j + 1] (first[] is the caller's prefix sum
// of the extents' chunk counts, n + 1 entries), found by bisection.  A workgroup of 256 lanes takes chunks
// blockIdx.x, blockIdx.x + gridDim.x, ...; a lane moves 16-byte pieces, loaded and stored at whatever alignment
// they have, and the lanes of the chunk's last piece move its odd bytes one by one.  No byte outside an extent's
// destination range is written.
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t kChunk = 16384, kLanes = 256;
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef v4u v4u_u __attribute__((aligned(1)));

__global__ __launch_bounds__(kLanes) void gather_kernel(const uint64_t* __restrict__ src, const uint64_t* __restrict__ dst,
                                                         const uint64_t* __restrict__ len,
                                                         const uint64_t* __restrict__ first, uint32_t n) {
  const uint64_t chunks = first[n];
  for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
    uint32_t lo = 0, hi = n;  // first[lo] <= c < first[hi]
    while (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (first[mid] <= c) lo = mid;
      else hi = mid;
    }
    const uint64_t at = (c - first[lo]) * kChunk;
    const uint64_t left = len[lo] - at;
    const uint32_t m = left < kChunk ? (uint32_t)left : kChunk;
    const uint8_t* s = reinterpret_cast<const uint8_t*>(src[lo]) + at;
    uint8_t* d = reinterpret_cast<uint8_t*>(dst[lo]) + at;
    for (uint32_t p = threadIdx.x; 16 * p + 16 <= m; p += kLanes)
      *(reinterpret_cast<v4u_u*>(d) + p) = *(reinterpret_cast<const v4u_u*>(s) + p);
    const uint32_t odd = m & 15u;
    if (threadIdx.x < odd) d[m - odd + threadIdx.x] = s[m - odd + threadIdx.x];
  }
}

}  // namespace

extern "C" {

// Chunk size, for the caller's prefix sum: extent j has (len[j] + chunk - 1) / chunk chunks.
uint32_t gathercopy_chunk(void) { return kChunk; }

// src, dst, len (n entries each) and first (n + 1) are device arrays of 64-bit words on `device`.  Asynchronous
// on `stream`; `groups` workgroups (a few per CU).
int gathercopy_launch(int device, const void* src, const void* dst, const void* len, const void* first, uint32_t n,
                      int groups, void* stream) {
  if (device < 0 || groups <= 0 || !src || !dst || !len || !first) return -1;
  if (n == 0) return 0;
  int prev = 0;
  if (hipGetDevice(&prev) != hipSuccess || hipSetDevice(device) != hipSuccess) return -2;
  hipLaunchKernelGGL(gather_kernel, dim3(groups), dim3(kLanes), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint64_t*>(src), static_cast<const uint64_t*>(dst),
                     static_cast<const uint64_t*>(len), static_cast<const uint64_t*>(first), n);
  const int rc = hipGetLastError() == hipSuccess ? 0 : -4;
  (void)hipSetDevice(prev);
  return rc;
}

}  // extern "C"
