// efes_objects_results.hip -- efes_objects_results: the sums and statuses a chain call left per extent, sorted
// out per object on the device: one 32-byte result per object (digest, status, verdict against an expected
// digest), the ascending list of the objects that are not in order, and four counters.  A translation unit, and
// so a code object, of its own, so that the code objects of the other .hip files are the ones they were without it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "efes_internal.hpp"
#include "efes_objects_rules.hpp"

namespace efes {

// ------------------------------------------------------------------ object results (efes_objects_results)
// Stream-ordered launches over the caller's scratch, every grid sized from an element count:
//   * a memset of fail[0, nobjects) to kResultsNone (all bits set);
//   * results_fail_kernel (one lane per extent, kResultsBlock per workgroup): a member whose status is not EFES_OK
//     looks its owner up (objects_owner, so only failed members search) and takes the 32-bit atomic minimum of its
//     index into fail[owner].  No lane loops over an object's members: one object may own all 2^20 extents.
//   * results_objects_kernel (one lane per object): results_object (efes_objects_rules.hpp) gives the eight words
//     of the result from fail[i], at most two statuses and one sum; the lane stores them as four 64-bit words;
//     the exclusive rank of its bad flag within the workgroup goes to rank[i] (bit 0: the flag), the workgroup's
//     count of each verdict to bcnt[4 b + v].
//   * results_bad_kernel (same grid, or one workgroup when no list is asked for): every workgroup sums the bad
//     counts of the workgroups before it (the second level of the scan) and each bad lane stores its own index at
//     bad[base + rank], so the list is ascending; the last workgroup sums bcnt[] into counts[0, 4), so counts[1]
//     + counts[2] is the scan's total by construction.  Two levels cover kResultsBlock^2 objects.
// Every index that forms an address is clamped: objects_owner returns an index of [0, nobjects), first[] is read
// only at [0, nobjects], the statuses and sums only at an index of [0, nextents) (results_object), and every lane
// checks its element index against the count before it loads or stores.  The only atomics are vector atomics on
// fail[]; no wave waits for another; no inline assembly.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage;
// profiles/objects_results/resources.txt): no scratch, no spills.
constexpr uint32_t kResultsBlock = 1024;  // lanes of a workgroup; two scan levels cover kResultsBlock^2
constexpr uint32_t kResultsWaves = kResultsBlock / 64;
static_assert((uint64_t)kResultsBlock * kResultsBlock >= EFES_OBJECTS_MAX, "two scan levels cover EFES_OBJECTS_MAX");

static inline uint32_t results_blocks(uint32_t n) { return (n + kResultsBlock - 1) / kResultsBlock; }

// The scratch: fail[nobjects], rank[nobjects], bcnt[4 * blocks].
struct ResultsScratch {
  uint32_t *fail, *rank, *bcnt;
};
static inline ResultsScratch results_scratch_of(void* scratch, uint32_t nobjects) {
  ResultsScratch S;
  S.fail = static_cast<uint32_t*>(scratch);
  S.rank = S.fail + nobjects;
  S.bcnt = S.rank + nobjects;
  return S;
}

size_t objects_results_scratch_bytes(uint32_t nobjects, uint32_t nextents) {
  if (nobjects > EFES_OBJECTS_MAX || nextents > EFES_OBJECTS_MAX) return 0;
  const size_t words = 2 * (size_t)nobjects + 4 * (size_t)results_blocks(nobjects);
  return ((words * 4 + 15) & ~(size_t)15) + 16;  // never 0 for counts the call takes
}

// Sum of v over the workgroup's kResultsBlock lanes, and this lane's exclusive prefix (wsum: kResultsWaves LDS
// words): objects_block_scan of efes_objects.hip with 32-bit sums.
__device__ uint32_t results_block_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off, 64);
    if (lane >= (uint32_t)off) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < kResultsWaves; ++k) {
    const uint32_t s = wsum[k];
    if (k < wave) base += s;
    tot += s;
  }
  __syncthreads();  // wsum may be written again
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(kResultsBlock) void results_fail_kernel(const uint32_t* __restrict__ first, uint32_t m, uint32_t n,
                                                                     const int32_t* __restrict__ status,
                                                                     uint32_t* __restrict__ fail) {
  const uint32_t j = blockIdx.x * kResultsBlock + threadIdx.x;
  if (j >= n || status[j] == EFES_OK) return;
  atomicMin(fail + objects_owner(first, m, j), j);  // m > 0: the launcher runs this for tables with objects only
}

__global__ __launch_bounds__(kResultsBlock) void results_objects_kernel(const uint32_t* __restrict__ first, uint32_t m, uint32_t n,
                                                                        const int32_t* __restrict__ status,
                                                                        const uint8_t* __restrict__ sums,
                                                                        const uint8_t* __restrict__ expected, uint32_t compare,
                                                                        const uint32_t* __restrict__ fail,
                                                                        uint64_t* __restrict__ results,
                                                                        uint32_t* __restrict__ rank, uint32_t* __restrict__ bcnt) {
  __shared__ uint32_t wsum[kResultsWaves];
  __shared__ uint32_t wcnt[kResultsWaves][4];
  const uint32_t i = blockIdx.x * kResultsBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t verdict = ~0u;  // a lane behind the last object counts for no verdict
  if (i < m) {
    uint32_t w[kResultWords];
    results_object(first, n, status, sums, expected, compare, i, n ? fail[i] : kResultsNone, w);
    verdict = w[7];
    if (results) {
      uint64_t* r = results + 4 * (size_t)i;
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = (uint64_t)w[2 * k] | ((uint64_t)w[2 * k + 1] << 32);
    }
  }
#pragma unroll
  for (uint32_t v = 0; v < 4; ++v) {
    const unsigned long long b = __ballot(verdict == v);
    if (lane == 0) wcnt[wave][v] = (uint32_t)__popcll(b);
  }
  const uint32_t bad = i < m && results_is_bad(verdict) ? 1u : 0u;
  uint32_t total;
  const uint32_t excl = results_block_scan(bad, wsum, &total);  // its barriers also publish wcnt
  if (i < m) rank[i] = (excl << 1) | bad;
  if (threadIdx.x < 4) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t k = 0; k < kResultsWaves; ++k) c += wcnt[k][threadIdx.x];
    bcnt[4 * blockIdx.x + threadIdx.x] = c;
  }
}

// Workgroup b of `blocks` (first_block + blockIdx.x): bad[base + rank] = i for its bad lanes, base = the bad
// counts of the workgroups before b; the last one also writes counts[0, 4).  blocks <= kResultsBlock.
__global__ __launch_bounds__(kResultsBlock) void results_bad_kernel(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ bcnt,
                                                                    uint32_t m, uint32_t blocks, uint32_t first_block,
                                                                    uint32_t* __restrict__ bad, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wsum[kResultsWaves];
  const uint32_t b = first_block + blockIdx.x, t = threadIdx.x;
  uint32_t c[4] = {0u, 0u, 0u, 0u};
  if (t < blocks) {
#pragma unroll
    for (int v = 0; v < 4; ++v) c[v] = bcnt[4 * t + v];
  }
  uint32_t base;
  (void)results_block_scan(t < b ? c[1] + c[2] : 0u, wsum, &base);
  if (bad) {
    const uint32_t i = b * kResultsBlock + t;
    if (i < m) {
      const uint32_t r = rank[i];
      if (r & 1u) bad[base + (r >> 1)] = i;  // base + rank < the number of bad objects <= m
    }
  }
  if (b + 1 != blocks) return;  // uniform
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    uint32_t total;
    (void)results_block_scan(c[v], wsum, &total);
    if (t == 0) counts[v] = total;
  }
}

#define EFES_RESULTS_LAUNCHED()              \
  do {                                       \
    const hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) return e_;         \
  } while (0)

hipError_t launch_objects_results(const efes_objects& in, const efes_results& req, void* scratch, hipStream_t s) {
  const uint32_t n = in.nextents, m = in.nobjects;
  clear_last_error();
  if (m == 0) return hipMemsetAsync(req.counts, 0, 4 * sizeof(uint32_t), s);
  const ResultsScratch S = results_scratch_of(scratch, m);
  const uint32_t ob = results_blocks(m);
  if (n) {
    const hipError_t e = hipMemsetAsync(S.fail, 0xFF, (size_t)m * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(results_fail_kernel, dim3(results_blocks(n)), dim3(kResultsBlock), 0, s, in.first, m, n,
                       (const int32_t*)in.status, S.fail);
    EFES_RESULTS_LAUNCHED();
  }
  hipLaunchKernelGGL(results_objects_kernel, dim3(ob), dim3(kResultsBlock), 0, s, in.first, m, n, (const int32_t*)in.status,
                     (const uint8_t*)in.sums, req.expected, req.compare, (const uint32_t*)S.fail,
                     reinterpret_cast<uint64_t*>(req.results), S.rank, S.bcnt);
  EFES_RESULTS_LAUNCHED();
  // without a list only the last workgroup has work: the counters
  hipLaunchKernelGGL(results_bad_kernel, dim3(req.bad ? ob : 1u), dim3(kResultsBlock), 0, s, (const uint32_t*)S.rank,
                     (const uint32_t*)S.bcnt, m, ob, req.bad ? 0u : ob - 1, req.bad, req.counts);
  return hipGetLastError();
}

}  // namespace efes
