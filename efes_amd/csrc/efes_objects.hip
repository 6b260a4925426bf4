// efes_objects.hip -- efes_objects_jobs: an object table (extents + object boundaries, in device memory)
// expanded on the device into the job array, the destination pointers and the record pointers that the
// chain calls take, and the gather layout.  A translation unit, and so a code object, of its own, so that
// the code objects of the other .hip files are the ones they were without it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "efes_internal.hpp"
#include "efes_objects_rules.hpp"

namespace efes {

// ------------------------------------------------------------------ object tables (efes_objects_jobs)
// Stream-ordered launches over the caller's scratch, every grid sized from an element count:
//   * objects_lengths_kernel (one lane per extent, kObjectsBlock per workgroup): the exclusive sum of the
//     lengths before each extent within its block (E[j]) and the block's sum (bsum[b]); zeroes layout[nobjects].
//   * objects_fix_kernel (same grid): every workgroup sums the bsum[] of the blocks before it and adds that
//     to its E[j]; the last one stores E[nextents], the sum of all.  Two levels, so kObjectsBlock^2 elements.
//   * objects_sizes_kernel + objects_fix_kernel (one lane per object; default layout only): the same scan
//     over the objects' sizes size[i] = E[first[i + 1]] - E[first[i]] rounded up to copy_align, into R[i].
//   * objects_layout_kernel (one lane per object; layout != NULL only): layout[i] = L[i], L = copy_offsets or
//     R; layout[nobjects] = L[last] + size[last] (default) or the 64-bit maximum of L[i] + size[i] (explicit
//     offsets), reduced over each wavefront by shuffles and then by one vector atomic per wavefront.
//   * objects_fill_kernel (one lane per extent, kObjectsFillBlock per workgroup): the owner by binary search
//     over first[0, nobjects) -- once per extent --, the seven words of the job into LDS, dst[j] and ckpt[j]
//     stored directly (one 64-bit word per lane, contiguous over the wavefront); after a barrier the
//     workgroup stores its 7 x kObjectsFillBlock job words in order, lane t the words t, t + 256, ..., so
//     every store instruction of the job array is contiguous over the wavefront too, instead of one 8-byte
//     word per 56-byte stride (DESIGN.md §4 "Object tables").
// Every index that forms an address is clamped: objects_owner returns an index of [0, nobjects), first[] is
// read only at [0, nobjects], E[] only at [0, nextents] (objects_bound), and every lane checks its element
// index against the count before it loads or stores.  No wave waits for another; no inline assembly.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage;
// profiles/objects_jobs/resources.txt): no scratch, no spills, 8 waves/SIMD for every kernel.
constexpr uint32_t kObjectsBlock = 1024;     // lanes of a scan workgroup; two levels cover kObjectsBlock^2
constexpr uint32_t kObjectsFillBlock = 256;  // extents per fill workgroup (14 KiB of job words in LDS)
static_assert((uint64_t)kObjectsBlock * kObjectsBlock >= EFES_OBJECTS_MAX, "two scan levels cover EFES_OBJECTS_MAX");

static inline uint32_t objects_blocks(uint32_t n) { return (n + kObjectsBlock - 1) / kObjectsBlock; }

// The scratch: E[nextents + 1], R[nobjects + 1], then the block sums of either scan.
struct ObjectsScratch {
  uint64_t *E, *R, *bsumE, *bsumR;
};
static inline ObjectsScratch objects_scratch_of(void* scratch, uint32_t nobjects, uint32_t nextents) {
  ObjectsScratch S;
  S.E = static_cast<uint64_t*>(scratch);
  S.R = S.E + ((size_t)nextents + 1);
  S.bsumE = S.R + ((size_t)nobjects + 1);
  S.bsumR = S.bsumE + objects_blocks(nextents);
  return S;
}

size_t objects_jobs_scratch_bytes(uint32_t nobjects, uint32_t nextents) {
  if (nobjects > EFES_OBJECTS_MAX || nextents > EFES_OBJECTS_MAX) return 0;
  const size_t words = ((size_t)nextents + 1) + ((size_t)nobjects + 1) + objects_blocks(nextents) + objects_blocks(nobjects);
  return (words * 8 + 15) & ~(size_t)15;
}

// Sum of v over the workgroup's kObjectsBlock lanes, and this lane's exclusive prefix (wsum: 16 LDS words);
// chain_block_scan of efes_kernels.hip with 64-bit sums, modulo 2^64.
__device__ uint64_t objects_block_scan(uint64_t v, uint64_t* wsum, uint64_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(inc, off, 64);
    if (lane >= (uint32_t)off) inc += o;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  uint64_t base = 0, tot = 0;
#pragma unroll
  for (uint32_t k = 0; k < kObjectsBlock / 64; ++k) {
    const uint64_t s = wsum[k];
    if (k < wave) base += s;
    tot += s;
  }
  __syncthreads();  // wsum may be written again
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(kObjectsBlock) void objects_lengths_kernel(const efes_extent* __restrict__ ext, uint32_t n,
                                                                        uint64_t* __restrict__ E, uint64_t* __restrict__ bsum,
                                                                        uint64_t* room) {
  __shared__ uint64_t wsum[kObjectsBlock / 64];
  const uint32_t j = blockIdx.x * kObjectsBlock + threadIdx.x;
  uint64_t total;
  const uint64_t excl = objects_block_scan(j < n ? ext[j].length : 0ull, wsum, &total);
  if (j < n) E[j] = excl;
  if (threadIdx.x == 0) {
    bsum[blockIdx.x] = total;
    if (blockIdx.x == 0 && room) *room = 0ull;
  }
}

// A[j] += the sums of the blocks before j's; A[n] = the sum of all.  gridDim.x <= kObjectsBlock.
__global__ __launch_bounds__(kObjectsBlock) void objects_fix_kernel(uint64_t* __restrict__ A, const uint64_t* __restrict__ bsum,
                                                                    uint32_t n) {
  __shared__ uint64_t wsum[kObjectsBlock / 64];
  uint64_t base;
  (void)objects_block_scan(threadIdx.x < blockIdx.x ? bsum[threadIdx.x] : 0ull, wsum, &base);
  const uint32_t j = blockIdx.x * kObjectsBlock + threadIdx.x;
  if (j < n) A[j] += base;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) A[n] = base + bsum[blockIdx.x];
}

// Bytes of object i < m: E at its two boundaries, both clamped into E[0, n].
__device__ __forceinline__ uint64_t objects_size(const uint32_t* __restrict__ first, const uint64_t* __restrict__ E, uint32_t i,
                                                 uint32_t n) {
  return E[objects_bound(first, i + 1, n)] - E[objects_bound(first, i, n)];
}

__global__ __launch_bounds__(kObjectsBlock) void objects_sizes_kernel(const uint32_t* __restrict__ first, uint32_t m, uint32_t n,
                                                                      const uint64_t* __restrict__ E, uint64_t align,
                                                                      uint64_t* __restrict__ R, uint64_t* __restrict__ bsum) {
  __shared__ uint64_t wsum[kObjectsBlock / 64];
  const uint32_t i = blockIdx.x * kObjectsBlock + threadIdx.x;
  uint64_t total;
  const uint64_t excl = objects_block_scan(i < m ? objects_round_up(objects_size(first, E, i, n), align) : 0ull, wsum, &total);
  if (i < m) R[i] = excl;
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// layout[i] = L[i]; layout[m], zeroed by an earlier launch, = the room.  E == NULL: no extents, every size 0.
__global__ __launch_bounds__(kObjectsBlock) void objects_layout_kernel(const uint32_t* __restrict__ first, uint32_t m, uint32_t n,
                                                                       const uint64_t* __restrict__ E,
                                                                       const uint64_t* __restrict__ L, bool explicit_offsets,
                                                                       uint64_t* __restrict__ layout) {
  const uint32_t i = blockIdx.x * kObjectsBlock + threadIdx.x;
  unsigned long long end = 0ull;
  if (i < m) {
    const uint64_t at = L ? L[i] : 0ull;
    layout[i] = at;
    end = at + (E ? objects_size(first, E, i, n) : 0ull);
    if (!explicit_offsets && i + 1 == m) layout[m] = end;
  }
  if (!explicit_offsets) return;  // uniform
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(end, off, 64);
    end = o > end ? o : end;
  }
  if ((threadIdx.x & 63u) == 0 && end) atomicMax(reinterpret_cast<unsigned long long*>(layout + m), end);
}

__global__ __launch_bounds__(kObjectsFillBlock) void objects_fill_kernel(const efes_objects in, const uint64_t* __restrict__ E,
                                                                         const uint64_t* __restrict__ L,
                                                                         uint64_t* __restrict__ jobs, uint64_t* __restrict__ dst,
                                                                         uint64_t* __restrict__ ckpt) {
  __shared__ uint64_t rec[kObjectsFillBlock * kJobWords];
  const uint32_t n = in.nextents, m = in.nobjects;
  const uint32_t j = blockIdx.x * kObjectsFillBlock + threadIdx.x;
  if (j < n) {
    const uint32_t i = objects_owner(in.first, m, j);
    const efes_extent e = in.extents[j];
    uint64_t* r = rec + threadIdx.x * kJobWords;
    r[0] = (uint64_t)(uintptr_t)in.data + e.offset;
    r[1] = e.length;
    r[2] = in.sha1 ? (uint64_t)(uintptr_t)(in.sha1 + i) : 0ull;
    r[3] = in.crc32 ? (uint64_t)(uintptr_t)(in.crc32 + i) : 0ull;
    r[4] = (uint64_t)(uintptr_t)in.sums + 24ull * j;
    r[5] = in.status ? (uint64_t)(uintptr_t)(in.status + j) : 0ull;
    r[6] = (uint64_t)objects_job_flags(in.first, m, i, j, in.flags);  // _reserved = 0 in the upper half
    if (ckpt) ckpt[j] = (uint64_t)(uintptr_t)(in.ckpt + j);
    if (dst) {
      const uint64_t at = m && L ? L[i] : 0ull;
      dst[j] = (uint64_t)(uintptr_t)in.copy_to + at + (E[j] - E[objects_bound(in.first, i, n)]);
    }
  }
  __syncthreads();
  const uint32_t base = blockIdx.x * (kObjectsFillBlock * kJobWords);  // < 7 * 2^20
  const uint32_t words = n * kJobWords;
#pragma unroll
  for (int k = 0; k < kJobWords; ++k) {
    const uint32_t w = k * kObjectsFillBlock + threadIdx.x;
    if (base + w < words) jobs[base + w] = rec[w];
  }
}

#define EFES_OBJECTS_LAUNCHED()        \
  do {                                 \
    const hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) return e_;   \
  } while (0)

hipError_t launch_objects_jobs(const efes_objects& in, const efes_objects_out& out, void* scratch, hipStream_t s) {
  const uint32_t n = in.nextents, m = in.nobjects;
  uint64_t* room = out.layout ? out.layout + m : nullptr;
  const bool explicit_offsets = in.copy_offsets != nullptr;
  clear_last_error();
  if (n == 0) {  // nothing for jobs; the layout of objects that all have no bytes
    if (!out.layout) return hipSuccess;
    const hipError_t e = hipMemsetAsync(room, 0, sizeof(uint64_t), s);
    if (e != hipSuccess || m == 0) return e;
    hipLaunchKernelGGL(objects_layout_kernel, dim3(objects_blocks(m)), dim3(kObjectsBlock), 0, s, (const uint32_t*)nullptr, m, 0u,
                       (const uint64_t*)nullptr, in.copy_offsets, explicit_offsets, out.layout);
    return hipGetLastError();
  }
  const ObjectsScratch S = objects_scratch_of(scratch, m, n);
  const uint32_t eb = objects_blocks(n), ob = objects_blocks(m);
  hipLaunchKernelGGL(objects_lengths_kernel, dim3(eb), dim3(kObjectsBlock), 0, s, in.extents, n, S.E, S.bsumE, room);
  EFES_OBJECTS_LAUNCHED();
  hipLaunchKernelGGL(objects_fix_kernel, dim3(eb), dim3(kObjectsBlock), 0, s, S.E, (const uint64_t*)S.bsumE, n);
  EFES_OBJECTS_LAUNCHED();
  const uint64_t* L = in.copy_offsets;
  if (!explicit_offsets && m && (out.layout || in.copy_to)) {
    hipLaunchKernelGGL(objects_sizes_kernel, dim3(ob), dim3(kObjectsBlock), 0, s, in.first, m, n, (const uint64_t*)S.E,
                       (uint64_t)objects_align_of(&in), S.R, S.bsumR);
    EFES_OBJECTS_LAUNCHED();
    hipLaunchKernelGGL(objects_fix_kernel, dim3(ob), dim3(kObjectsBlock), 0, s, S.R, (const uint64_t*)S.bsumR, m);
    EFES_OBJECTS_LAUNCHED();
    L = S.R;
  }
  if (out.layout && m) {
    hipLaunchKernelGGL(objects_layout_kernel, dim3(ob), dim3(kObjectsBlock), 0, s, in.first, m, n, (const uint64_t*)S.E, L,
                       explicit_offsets, out.layout);
    EFES_OBJECTS_LAUNCHED();
  }
  hipLaunchKernelGGL(objects_fill_kernel, dim3((n + kObjectsFillBlock - 1) / kObjectsFillBlock), dim3(kObjectsFillBlock), 0, s, in,
                     (const uint64_t*)S.E, L, reinterpret_cast<uint64_t*>(out.jobs),
                     in.copy_to ? reinterpret_cast<uint64_t*>(out.dst) : nullptr,
                     in.ckpt ? reinterpret_cast<uint64_t*>(out.ckpt) : nullptr);
  return hipGetLastError();
}

}  // namespace efes
