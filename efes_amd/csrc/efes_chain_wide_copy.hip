// efes_chain_wide_copy.hip -- the wide chain walk that also gathers (efes_hash_chain_wide_copy): a translation
// unit, and so a code object, of its own, so that the code objects of efes_kernels.hip and efes_chain_wide.hip
// are the ones they were without it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "efes_internal.hpp"
#include "efes_chain_wide_device.hpp"

namespace efes {

// ------------------------------------------------------------------ wide walk with copy (efes_hash_chain_wide_copy)
// efes_chain_wide_body.inc with kCopy set: the walk of hash_chain_wide_kernel with three
// stores added, all under the walk's `go` predicate and dsts[j] != NULL -- the head bytes beside the loads that
// complete x, every whole block as four 16-byte stores from the register buffer it is hashed from
// (wide_bulk_copy), the tail bytes one by one.  Draw, rounds, validity, Sum, records, wide_pace and the early
// exit of the waves the chain count cannot fill are the walk's; no wave waits for another, and there is no
// barrier, LDS-DMA or inline assembly that the walk does not have.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage;
// profiles/hash_chain_wide_copy/resources.txt):
//   hash_chain_wide_copy_kernel<false>  153 VGPRs, 90 SGPRs, 65 584 B static LDS, no scratch, no spills, 3 waves/SIMD
//   hash_chain_wide_copy_kernel<true>   153 VGPRs, 98 SGPRs, 65 584 B static LDS, no scratch, no spills, 3 waves/SIMD
//   no AGPRs; + 17 408 B of dynamic LDS per wave per SIMD, as the walk.  Six VGPRs more than hash_chain_wide_kernel
//   (the destination pointer, the copy predicate, the store addresses), under the 170 that three waves per SIMD allow;
//   the launcher asks the runtime what fits (launch_wide_walk) and does not assume the three.
template <bool kCkpt>
__global__ __launch_bounds__(64 * kWideWaves * kWideMaxWps, 1) void hash_chain_wide_copy_kernel(
    const efes_job* __restrict__ jobs, uint32_t njobs, const Tables* __restrict__ tabs, void* scratch,
    efes_checkpoint* const* __restrict__ ckpt, void* const* __restrict__ dsts) {
  __shared__ __attribute__((aligned(16))) WideLDS L;
  extern __shared__ __attribute__((aligned(16))) uint8_t chain_wide_xs[];  // blockDim.x x kXStride
  constexpr bool kCopy = true;
#include "efes_chain_wide_body.inc"
}

hipError_t launch_hash_chain_wide_copy(const efes_job* jobs, void* const* dsts, uint32_t njobs,
                                       efes_checkpoint* const* ckpt, void* scratch, const Tables* tabs, int cus,
                                       hipStream_t s) {
  if (njobs == 0) return hipSuccess;
  const hipError_t e = launch_hash_chain_prep(jobs, njobs, scratch, s);
  if (e != hipSuccess) return e;
  if (ckpt)
    return launch_wide_walk<hash_chain_wide_copy_kernel<true>>(njobs, cus, s, jobs, njobs, tabs, scratch, ckpt, dsts);
  return launch_wide_walk<hash_chain_wide_copy_kernel<false>>(njobs, cus, s, jobs, njobs, tabs, scratch,
                                                              (efes_checkpoint* const*)nullptr, dsts);
}

}  // namespace efes
