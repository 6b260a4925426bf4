// efes_objects_order.hip -- efes_objects_order: the longest-first ranking of an object table's objects, sorted
// on the device; and efes_objects_jobs_ordered: efes_objects_jobs that emits the objects in a given order.  A
// translation unit, and so a code object, of its own, so that the code objects of the other .hip files are the
// ones they were without it; the scan helpers of efes_objects.hip are restated here for that reason.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "efes_internal.hpp"
#include "efes_objects_rules.hpp"

namespace efes {

// ------------------------------------------------------------------ shared: two-level 64-bit scans
// Stream-ordered launches over the caller's scratch, every grid sized from an element count.  Every lane checks
// its element index against the count before it loads or stores; first[] is read only at [0, nobjects] and
// clamped (objects_bound) before it indexes E[0, nextents]; order[] is clamped (order_object) before it indexes
// anything; a scatter position is checked against nobjects before the store.  The only atomics are vector
// atomics: one 64-bit OR per wavefront on the sort's `diff` word, 32-bit adds in LDS.  No wave waits for
// another; no inline assembly.  Resources (hipcc -O3 --offload-arch=gfx950
// -Rpass-analysis=kernel-resource-usage; profiles/objects_order/resources.txt): no scratch, no spills.
constexpr uint32_t kOrderBlock = 1024;  // lanes of a scan workgroup; two levels cover kOrderBlock^2
constexpr uint32_t kOrderWaves = kOrderBlock / 64;
constexpr uint32_t kOrderTile = kOrderBlock;  // pairs of one sort workgroup: one per lane
constexpr uint32_t kOrderRadix = 256;         // order_digit: eight digits of eight bits
constexpr uint32_t kOrderDigits = 8;
constexpr uint32_t kOrderFillBlock = 256;  // slots per fill workgroup (14 KiB of job words in LDS)
static_assert((uint64_t)kOrderBlock * kOrderBlock >= EFES_OBJECTS_MAX, "two scan levels cover EFES_OBJECTS_MAX");
static_assert((uint64_t)kOrderRadix * (EFES_OBJECTS_MAX / kOrderTile) <= (uint64_t)kOrderBlock * kOrderBlock,
              "two scan levels cover the digit counts of every tile");

static inline uint32_t order_blocks(uint32_t n) { return (n + kOrderBlock - 1) / kOrderBlock; }
static inline size_t order_align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// Sum of v over the workgroup's kOrderBlock lanes, and this lane's exclusive prefix (wsum: kOrderWaves LDS
// words), modulo 2^64 or 2^32: objects_block_scan of efes_objects.hip.
template <typename T>
__device__ T order_block_scan(T v, T* wsum, T* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(inc, off, 64);
    if (lane >= (uint32_t)off) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < kOrderWaves; ++k) {
    const T s = wsum[k];
    if (k < wave) base += s;
    tot += s;
  }
  __syncthreads();  // wsum may be written again
  *total = tot;
  return base + inc - v;
}

// E[j] = the lengths before j within its block; bsum[b] = the block's sum.
__global__ __launch_bounds__(kOrderBlock) void order_lengths_kernel(const efes_extent* __restrict__ ext, uint32_t n,
                                                                    unsigned long long* __restrict__ E,
                                                                    unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long wsum[kOrderWaves];
  const uint32_t j = blockIdx.x * kOrderBlock + threadIdx.x;
  unsigned long long total;
  const unsigned long long excl = order_block_scan<unsigned long long>(j < n ? ext[j].length : 0ull, wsum, &total);
  if (j < n) E[j] = excl;
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// A[j] += the sums of the blocks before j's; A[n] = the sum of all.  gridDim.x <= kOrderBlock.
__global__ __launch_bounds__(kOrderBlock) void order_fix_kernel(unsigned long long* __restrict__ A,
                                                                const unsigned long long* __restrict__ bsum, uint32_t n) {
  __shared__ unsigned long long wsum[kOrderWaves];
  unsigned long long base;
  (void)order_block_scan<unsigned long long>(threadIdx.x < blockIdx.x ? bsum[threadIdx.x] : 0ull, wsum, &base);
  const uint32_t j = blockIdx.x * kOrderBlock + threadIdx.x;
  if (j < n) A[j] += base;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) A[n] = base + bsum[blockIdx.x];
}

#define EFES_ORDER_LAUNCHED()                \
  do {                                       \
    const hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) return e_;         \
  } while (0)

// E[0, n] of the table's lengths, n > 0.
static hipError_t order_scan_lengths(const efes_objects& in, unsigned long long* E, unsigned long long* bsum, hipStream_t s) {
  const uint32_t n = in.nextents, eb = order_blocks(n);
  hipLaunchKernelGGL(order_lengths_kernel, dim3(eb), dim3(kOrderBlock), 0, s, in.extents, n, E, bsum);
  EFES_ORDER_LAUNCHED();
  hipLaunchKernelGGL(order_fix_kernel, dim3(eb), dim3(kOrderBlock), 0, s, E, (const unsigned long long*)bsum, n);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the order (efes_objects_order)
// A stable LSD radix sort of (key = ~size, value = object index) pairs, from the identity, radix 256:
//   * order_lengths_kernel + order_fix_kernel: E, the scan of the lengths (tables with extents);
//   * a memset of `diff`, then order_keys_kernel (one lane per object): key[i] = ~size[i], value[i] = i into
//     buffer 0, and the OR over all i of key[i] ^ key[0] into `diff` (reduced over each wavefront by shuffles,
//     then one vector atomic per wavefront): digit d is shared by all keys exactly when byte d of diff is 0;
//   * for each digit d = 0..7 three launches that return at once where all keys share the digit.  The buffer a
//     pass reads is the parity of the number of digits below d that were NOT skipped (order_pass), so nothing
//     is read back:
//       - order_count_kernel (one lane per pair, kOrderTile per workgroup): counts[v * tiles + t] = the pairs of
//         tile t with digit value v;
//       - order_scan_kernel (one lane per count): the exclusive sums within each block of kOrderBlock counts,
//         in place, and each block's sum;
//       - order_scatter_kernel (grid of the count kernel): the second scan level over the block sums, then
//         every pair goes to (pairs with a smaller digit value) + (pairs of that value in earlier tiles) + (its
//         rank among the pairs of that value in its tile, in index order: whole wavefronts before it by a table
//         in LDS, lanes before it by a match over the wavefront's ballots).  Stable.
//   * order_copy_kernel: the values of the buffer the last pass wrote go to order[].
// The number of launches is fixed by the counts; what they do is decided on the device.
struct OrderScratch {
  unsigned long long *E, *bsumE, *key[2], *diff;
  uint32_t *val[2], *counts, *csum;
};
static inline uint32_t order_tiles(uint32_t m) { return (m + kOrderTile - 1) / kOrderTile; }

// The 64-bit words first: diff, E[nextents + 1], the block sums of its scan, the two key buffers; then the 32-bit
// ones: the two value buffers, the digit counts and the block sums of their scan.
static inline size_t order_words64(uint32_t nobjects, uint32_t nextents) {
  return 1 + ((size_t)nextents + 1) + order_blocks(nextents) + 2 * (size_t)nobjects;
}
static inline OrderScratch order_scratch_of(void* scratch, uint32_t nobjects, uint32_t nextents) {
  OrderScratch S;
  S.diff = static_cast<unsigned long long*>(scratch);
  S.E = S.diff + 1;
  S.bsumE = S.E + ((size_t)nextents + 1);
  S.key[0] = S.bsumE + order_blocks(nextents);
  S.key[1] = S.key[0] + nobjects;
  S.val[0] = reinterpret_cast<uint32_t*>(S.key[1] + nobjects);
  S.val[1] = S.val[0] + nobjects;
  S.counts = S.val[1] + nobjects;
  S.csum = S.counts + kOrderRadix * order_tiles(nobjects);
  return S;
}

size_t objects_order_scratch_bytes(uint32_t nobjects, uint32_t nextents) {
  if (nobjects > EFES_OBJECTS_MAX || nextents > EFES_OBJECTS_MAX) return 0;
  const uint32_t ncounts = kOrderRadix * order_tiles(nobjects);
  const size_t words32 = 2 * (size_t)nobjects + ncounts + order_blocks(ncounts);
  return order_align16(order_words64(nobjects, nextents) * 8 + words32 * 4);  // never 0: the diff word is always there
}

// What pass d does, from the diff word: whether it runs, and which buffer it reads.
struct OrderPass {
  bool active;
  uint32_t src;
};
__device__ __forceinline__ OrderPass order_pass(unsigned long long diff, uint32_t d) {
  OrderPass p;
  uint32_t before = 0;
#pragma unroll
  for (uint32_t k = 0; k < kOrderDigits; ++k)
    if (k < d && order_digit(diff, k)) ++before;
  p.active = d < kOrderDigits && order_digit(diff, d < kOrderDigits ? d : 0u) != 0;  // d == kOrderDigits: the parity of all
  p.src = before & 1u;
  return p;
}

__global__ __launch_bounds__(kOrderBlock) void order_keys_kernel(const uint32_t* __restrict__ first, uint32_t m, uint32_t n,
                                                                 const unsigned long long* __restrict__ E,
                                                                 unsigned long long* __restrict__ key, uint32_t* __restrict__ val,
                                                                 unsigned long long* diff) {
  const uint32_t i = blockIdx.x * kOrderBlock + threadIdx.x;
  unsigned long long x = 0ull;
  if (i < m) {
    const unsigned long long k = order_key(order_size(first, (const uint64_t*)E, i, n));
    key[i] = k;
    val[i] = i;
    x = k ^ order_key(order_size(first, (const uint64_t*)E, 0u, n));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x |= __shfl_xor(x, off, 64);
  if ((threadIdx.x & 63u) == 0 && x) atomicOr(diff, x);
}

// The lanes of this wavefront, among those of `valid`, whose digit value equals this lane's.
__device__ __forceinline__ unsigned long long order_match(uint32_t v, unsigned long long valid) {
  unsigned long long same = valid;
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b) {
    const unsigned long long set = __ballot((v >> b) & 1u);
    same &= ((v >> b) & 1u) ? set : ~set;
  }
  return same;
}

__global__ __launch_bounds__(kOrderBlock) void order_count_kernel(const unsigned long long* key0, const unsigned long long* key1,
                                                                  uint32_t m, uint32_t tiles, uint32_t d,
                                                                  const unsigned long long* __restrict__ diff,
                                                                  uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[kOrderRadix];
  const OrderPass p = order_pass(*diff, d);
  if (!p.active) return;  // uniform
  const unsigned long long* key = p.src ? key1 : key0;
  if (threadIdx.x < kOrderRadix) hist[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * kOrderTile + threadIdx.x, lane = threadIdx.x & 63u;
  const bool have = i < m;
  const uint32_t v = have ? order_digit(key[i], d) : 0u;
  const unsigned long long same = order_match(v, __ballot(have));
  if (have && (same & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&hist[v], (uint32_t)__popcll(same));  // the group's first lane
  __syncthreads();
  if (threadIdx.x < kOrderRadix && blockIdx.x < tiles) counts[threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

__global__ __launch_bounds__(kOrderBlock) void order_scan_kernel(uint32_t* __restrict__ counts, uint32_t ncounts, uint32_t d,
                                                                 const unsigned long long* __restrict__ diff,
                                                                 uint32_t* __restrict__ csum) {
  __shared__ uint32_t wsum[kOrderWaves];
  if (!order_pass(*diff, d).active) return;  // uniform
  const uint32_t c = blockIdx.x * kOrderBlock + threadIdx.x;
  uint32_t total;
  const uint32_t excl = order_block_scan<uint32_t>(c < ncounts ? counts[c] : 0u, wsum, &total);
  if (c < ncounts) counts[c] = excl;
  if (threadIdx.x == 0) csum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kOrderBlock) void order_scatter_kernel(unsigned long long* key0, unsigned long long* key1,
                                                                    uint32_t* val0, uint32_t* val1, uint32_t m, uint32_t tiles,
                                                                    uint32_t d, const unsigned long long* __restrict__ diff,
                                                                    const uint32_t* __restrict__ counts,
                                                                    const uint32_t* __restrict__ csum) {
  __shared__ uint32_t wsum[kOrderWaves];
  __shared__ uint32_t cpre[kOrderBlock];               // the block sums of the counts' scan, scanned
  __shared__ uint32_t gbase[kOrderRadix];              // where this tile's pairs of each digit value begin
  __shared__ uint32_t wtab[kOrderWaves][kOrderRadix];  // the pairs of each value in each wavefront, then in those before it
  const OrderPass p = order_pass(*diff, d);
  if (!p.active) return;  // uniform
  const unsigned long long* key = p.src ? key1 : key0;
  const uint32_t* val = p.src ? val1 : val0;
  unsigned long long* key_to = p.src ? key0 : key1;
  uint32_t* val_to = p.src ? val0 : val1;
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t ncounts = kOrderRadix * tiles, cblocks = (ncounts + kOrderBlock - 1) / kOrderBlock;  // <= kOrderBlock
  uint32_t unused;
  cpre[t] = order_block_scan<uint32_t>(t < cblocks ? csum[t] : 0u, wsum, &unused);
  for (uint32_t k = t; k < kOrderWaves * kOrderRadix; k += kOrderBlock) (&wtab[0][0])[k] = 0u;
  __syncthreads();
  if (t < kOrderRadix) {
    const uint32_t c = t * tiles + blockIdx.x;  // < ncounts: blockIdx.x < tiles
    gbase[t] = c < ncounts ? counts[c] + cpre[c / kOrderBlock] : 0u;
  }
  const uint32_t i = blockIdx.x * kOrderTile + t;
  const bool have = i < m;
  unsigned long long k = 0ull;
  uint32_t x = 0u;
  if (have) {
    k = key[i];
    x = val[i];
  }
  const uint32_t v = have ? order_digit(k, d) : 0u;
  const unsigned long long same = order_match(v, __ballot(have));
  const uint32_t before = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
  if (have && before == 0u) wtab[wave][v] = (uint32_t)__popcll(same);  // one lane per value and wavefront
  __syncthreads();
  if (t < kOrderRadix) {  // wtab[w][t] = the pairs of value t in the wavefronts before w
    uint32_t at = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kOrderWaves; ++w) {
      const uint32_t c = wtab[w][t];
      wtab[w][t] = at;
      at += c;
    }
  }
  __syncthreads();
  if (have) {
    const uint32_t to = gbase[v] + wtab[wave][v] + before;
    if (to < m) {  // always, for counts that this launch's own count pass made
      key_to[to] = k;
      val_to[to] = x;
    }
  }
}

__global__ __launch_bounds__(kOrderBlock) void order_copy_kernel(const uint32_t* val0, const uint32_t* val1, uint32_t m,
                                                                 const unsigned long long* __restrict__ diff,
                                                                 uint32_t* __restrict__ order) {
  const uint32_t r = blockIdx.x * kOrderBlock + threadIdx.x;
  const uint32_t* val = order_pass(*diff, kOrderDigits).src ? val1 : val0;  // the parity of all the passes that ran
  if (r < m) {
    const uint32_t i = val[r];
    order[r] = i < m ? i : m - 1;
  }
}

hipError_t launch_objects_order(const efes_objects& in, uint32_t* order, void* scratch, hipStream_t s) {
  const uint32_t n = in.nextents, m = in.nobjects;
  clear_last_error();
  if (m == 0) return hipSuccess;
  const OrderScratch S = order_scratch_of(scratch, m, n);
  hipError_t e = hipMemsetAsync(S.diff, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  if (n) {
    e = order_scan_lengths(in, S.E, S.bsumE, s);
    if (e != hipSuccess) return e;
  }
  const uint32_t ob = order_blocks(m), tiles = order_tiles(m), ncounts = kOrderRadix * tiles;
  hipLaunchKernelGGL(order_keys_kernel, dim3(ob), dim3(kOrderBlock), 0, s, in.first, m, n, (const unsigned long long*)S.E, S.key[0],
                     S.val[0], S.diff);
  EFES_ORDER_LAUNCHED();
  for (uint32_t d = 0; d < kOrderDigits; ++d) {
    hipLaunchKernelGGL(order_count_kernel, dim3(tiles), dim3(kOrderBlock), 0, s, (const unsigned long long*)S.key[0],
                       (const unsigned long long*)S.key[1], m, tiles, d, (const unsigned long long*)S.diff, S.counts);
    EFES_ORDER_LAUNCHED();
    hipLaunchKernelGGL(order_scan_kernel, dim3(order_blocks(ncounts)), dim3(kOrderBlock), 0, s, S.counts, ncounts, d,
                       (const unsigned long long*)S.diff, S.csum);
    EFES_ORDER_LAUNCHED();
    hipLaunchKernelGGL(order_scatter_kernel, dim3(tiles), dim3(kOrderBlock), 0, s, S.key[0], S.key[1], S.val[0], S.val[1], m, tiles,
                       d, (const unsigned long long*)S.diff, (const uint32_t*)S.counts, (const uint32_t*)S.csum);
    EFES_ORDER_LAUNCHED();
  }
  hipLaunchKernelGGL(order_copy_kernel, dim3(ob), dim3(kOrderBlock), 0, s, (const uint32_t*)S.val[0], (const uint32_t*)S.val[1], m,
                     (const unsigned long long*)S.diff, order);
  return hipGetLastError();
}

// ------------------------------------------------------------------ the ordered builder (efes_objects_jobs_ordered)
// efes_objects_jobs (efes_objects.hip) with the objects emitted in a given order.  The scans of the lengths (E)
// and of the rounded sizes (R) and the layout pass are the builder's, restated; added are
//   * ordered_counts_kernel + order_fix_kernel (one lane per rank): J, the scan of cnt(order[r]);
//   * ordered_first_kernel (one lane per rank, job_first != NULL only): job_first[r] = min(J[r], nextents);
//   * ordered_fill_kernel (one lane per output SLOT, kOrderFillBlock per workgroup): the rank by binary search
//     over J[0, nobjects), the object and the extent of the slot (order_slot), the seven words of the job into
//     LDS, dst[k] and ckpt[k] stored directly; after a barrier the workgroup stores its 7 x kOrderFillBlock job
//     words in order, lane t the words t, t + 256, ..., contiguous over the wavefront, as objects_fill_kernel does.
struct OrderedScratch {
  unsigned long long *E, *R, *J, *bsumE, *bsumR, *bsumJ;
};
static inline OrderedScratch ordered_scratch_of(void* scratch, uint32_t nobjects, uint32_t nextents) {
  OrderedScratch S;
  S.E = static_cast<unsigned long long*>(scratch);
  S.R = S.E + ((size_t)nextents + 1);
  S.J = S.R + ((size_t)nobjects + 1);
  S.bsumE = S.J + ((size_t)nobjects + 1);
  S.bsumR = S.bsumE + order_blocks(nextents);
  S.bsumJ = S.bsumR + order_blocks(nobjects);
  return S;
}

size_t objects_jobs_ordered_scratch_bytes(uint32_t nobjects, uint32_t nextents) {
  if (nobjects > EFES_OBJECTS_MAX || nextents > EFES_OBJECTS_MAX) return 0;
  const size_t words = ((size_t)nextents + 1) + 2 * ((size_t)nobjects + 1) + order_blocks(nextents) + 2 * (size_t)order_blocks(nobjects);
  return order_align16(words * 8);  // never 0: E[nextents], R[nobjects] and J[nobjects] are always there
}

__global__ __launch_bounds__(kOrderBlock) void ordered_sizes_kernel(const uint32_t* __restrict__ first, uint32_t m, uint32_t n,
                                                                    const unsigned long long* __restrict__ E,
                                                                    unsigned long long align, unsigned long long* __restrict__ R,
                                                                    unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long wsum[kOrderWaves];
  const uint32_t i = blockIdx.x * kOrderBlock + threadIdx.x;
  unsigned long long total;
  const unsigned long long size = i < m ? objects_round_up(order_size(first, (const uint64_t*)E, i, n), align) : 0ull;
  const unsigned long long excl = order_block_scan<unsigned long long>(size, wsum, &total);
  if (i < m) R[i] = excl;
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// layout[i] = L[i]; layout[m], zeroed by an earlier memset, = the room.  n == 0: no extents, every size 0.
__global__ __launch_bounds__(kOrderBlock) void ordered_layout_kernel(const uint32_t* __restrict__ first, uint32_t m, uint32_t n,
                                                                     const unsigned long long* __restrict__ E,
                                                                     const unsigned long long* __restrict__ L,
                                                                     bool explicit_offsets, unsigned long long* __restrict__ layout) {
  const uint32_t i = blockIdx.x * kOrderBlock + threadIdx.x;
  unsigned long long end = 0ull;
  if (i < m) {
    const unsigned long long at = L ? L[i] : 0ull;
    layout[i] = at;
    end = at + order_size(first, (const uint64_t*)E, i, n);
    if (!explicit_offsets && i + 1 == m) layout[m] = end;
  }
  if (!explicit_offsets) return;  // uniform
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(end, off, 64);
    end = o > end ? o : end;
  }
  if ((threadIdx.x & 63u) == 0 && end) atomicMax(layout + m, end);
}

__global__ __launch_bounds__(kOrderBlock) void ordered_counts_kernel(const uint32_t* __restrict__ first,
                                                                     const uint32_t* __restrict__ order, uint32_t m, uint32_t n,
                                                                     unsigned long long* __restrict__ J,
                                                                     unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long wsum[kOrderWaves];
  const uint32_t r = blockIdx.x * kOrderBlock + threadIdx.x;
  unsigned long long total;
  const unsigned long long cnt = r < m ? order_count(first, order_object(order, m, r), n) : 0u;
  const unsigned long long excl = order_block_scan<unsigned long long>(cnt, wsum, &total);
  if (r < m) J[r] = excl;
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kOrderBlock) void ordered_first_kernel(const unsigned long long* __restrict__ J, uint32_t m, uint32_t n,
                                                                    uint32_t* __restrict__ job_first) {
  const uint32_t r = blockIdx.x * kOrderBlock + threadIdx.x;
  if (r <= m) job_first[r] = order_job_first(J[r], n);
}

__global__ __launch_bounds__(kOrderFillBlock) void ordered_fill_kernel(const efes_objects in, const uint32_t* __restrict__ order,
                                                                       const unsigned long long* __restrict__ E,
                                                                       const unsigned long long* __restrict__ L,
                                                                       const unsigned long long* __restrict__ J,
                                                                       unsigned long long* __restrict__ jobs,
                                                                       unsigned long long* __restrict__ dst,
                                                                       unsigned long long* __restrict__ ckpt) {
  __shared__ uint64_t rec[kOrderFillBlock * kJobWords];
  const uint32_t n = in.nextents, m = in.nobjects;
  const uint32_t k = blockIdx.x * kOrderFillBlock + threadIdx.x;
  if (k < n) {
    const OrderSlot at = order_slot(in.first, order, (const uint64_t*)J, m, n, k);
    order_job_words(in, at.i, at.j, rec + threadIdx.x * kJobWords);
    if (ckpt) ckpt[k] = (unsigned long long)(uintptr_t)(in.ckpt + at.j);
    if (dst) dst[k] = order_job_dst(in, (const uint64_t*)E, (const uint64_t*)L, at.i, at.j);
  }
  __syncthreads();
  const uint32_t base = blockIdx.x * (kOrderFillBlock * kJobWords);  // < 7 * 2^20
  const uint32_t words = n * kJobWords;
#pragma unroll
  for (int w = 0; w < kJobWords; ++w) {
    const uint32_t at = w * kOrderFillBlock + threadIdx.x;
    if (base + at < words) jobs[base + at] = rec[at];
  }
}

hipError_t launch_objects_jobs_ordered(const efes_objects& in, const efes_objects_out& out, const uint32_t* order,
                                       uint32_t* job_first, void* scratch, hipStream_t s) {
  const uint32_t n = in.nextents, m = in.nobjects;
  unsigned long long* layout = reinterpret_cast<unsigned long long*>(out.layout);
  const unsigned long long* offsets = reinterpret_cast<const unsigned long long*>(in.copy_offsets);
  const bool explicit_offsets = in.copy_offsets != nullptr;
  const uint32_t ob = order_blocks(m);
  clear_last_error();
  hipError_t e;
  if (layout) {  // the room: the layout pass writes it (default) or raises it (explicit offsets)
    e = hipMemsetAsync(layout + m, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
  }
  if (n == 0) {  // nothing for jobs; every rank begins at slot 0; the layout of objects that all have no bytes
    if (job_first) {
      e = hipMemsetAsync(job_first, 0, ((size_t)m + 1) * sizeof(uint32_t), s);
      if (e != hipSuccess) return e;
    }
    if (!layout || m == 0) return hipSuccess;
    hipLaunchKernelGGL(ordered_layout_kernel, dim3(ob), dim3(kOrderBlock), 0, s, (const uint32_t*)nullptr, m, 0u,
                       (const unsigned long long*)nullptr, offsets, explicit_offsets, layout);
    return hipGetLastError();
  }
  const OrderedScratch S = ordered_scratch_of(scratch, m, n);
  e = order_scan_lengths(in, S.E, S.bsumE, s);
  if (e != hipSuccess) return e;
  const unsigned long long* L = offsets;
  if (!explicit_offsets && m && (layout || in.copy_to)) {
    hipLaunchKernelGGL(ordered_sizes_kernel, dim3(ob), dim3(kOrderBlock), 0, s, in.first, m, n, (const unsigned long long*)S.E,
                       (unsigned long long)objects_align_of(&in), S.R, S.bsumR);
    EFES_ORDER_LAUNCHED();
    hipLaunchKernelGGL(order_fix_kernel, dim3(ob), dim3(kOrderBlock), 0, s, S.R, (const unsigned long long*)S.bsumR, m);
    EFES_ORDER_LAUNCHED();
    L = S.R;
  }
  if (layout && m) {
    hipLaunchKernelGGL(ordered_layout_kernel, dim3(ob), dim3(kOrderBlock), 0, s, in.first, m, n, (const unsigned long long*)S.E, L,
                       explicit_offsets, layout);
    EFES_ORDER_LAUNCHED();
  }
  if (m) {
    hipLaunchKernelGGL(ordered_counts_kernel, dim3(ob), dim3(kOrderBlock), 0, s, in.first, order, m, n, S.J, S.bsumJ);
    EFES_ORDER_LAUNCHED();
    hipLaunchKernelGGL(order_fix_kernel, dim3(ob), dim3(kOrderBlock), 0, s, S.J, (const unsigned long long*)S.bsumJ, m);
    EFES_ORDER_LAUNCHED();
    if (job_first) {
      hipLaunchKernelGGL(ordered_first_kernel, dim3(order_blocks(m + 1)), dim3(kOrderBlock), 0, s, (const unsigned long long*)S.J, m, n,
                         job_first);
      EFES_ORDER_LAUNCHED();
    }
  } else if (job_first) {
    e = hipMemsetAsync(job_first, 0, sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(ordered_fill_kernel, dim3((n + kOrderFillBlock - 1) / kOrderFillBlock), dim3(kOrderFillBlock), 0, s, in, order,
                     (const unsigned long long*)S.E, L, (const unsigned long long*)S.J, reinterpret_cast<unsigned long long*>(out.jobs),
                     in.copy_to ? reinterpret_cast<unsigned long long*>(out.dst) : nullptr,
                     in.ckpt ? reinterpret_cast<unsigned long long*>(out.ckpt) : nullptr);
  return hipGetLastError();
}

}  // namespace efes
