// efes_chain_wide.hip -- the wide chain walk (efes_hash_chain_wide): a translation unit, and so a code object,
// of its own, so that the code object of efes_kernels.hip is the one it was without this walk.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "efes_internal.hpp"
#include "efes_chain_wide_device.hpp"

namespace efes {

// ------------------------------------------------------------------ wide walk (efes_hash_chain_wide)
// The walk itself is efes_chain_wide_body.inc, which describes it; the copying walk (efes_hash_chain_wide_copy)
// includes the same body, with kCopy set, in efes_chain_wide_copy.hip.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage;
// profiles/hash_chain_wide/resources.txt):
//   hash_chain_wide_kernel<false>  147 VGPRs, 84 SGPRs, 65 584 B static LDS, no scratch, no spills, 3 waves/SIMD
//   hash_chain_wide_kernel<true>   147 VGPRs, 90 SGPRs, 65 584 B static LDS, no scratch, no spills, 3 waves/SIMD
//   no AGPRs; + 17 408 B of dynamic LDS per wave per SIMD (117 808 B at three), so one workgroup per CU.
// wide_kernel has 138 VGPRs: the per-lane chain bookkeeping (cursor, end, the members' flags, the state
// pointers kept across the rounds) costs nine and stays under the 170 that three waves per SIMD allow, so
// none of it was moved to LDS.  The launcher asks the runtime what fits and does not assume the three; on
// the MI355X it gets the three (workgroups of 512 and 768 lanes seen in the runtime's launch log for 98 945
// and 209 780 jobs).
// The walk has this translation unit, and so a code object, to itself.  In one code object with the other
// kernels it left their instructions, registers and LDS as they were and still slowed the grouped walks on
// 4096 objects x 64 x 4 KiB by 2.5 % (efes_hash_chain_mode) and 6.5 % (efes_hash_chain_checkpoints), measured
// against the tree without it on one machine; with the walk here the .text of efes_kernels.hip's code object
// is byte for byte what it is without the walk (DESIGN.md §4 "Chained SHA-1 + CRC, wide walk").  The shared
// __forceinline__ helpers live in efes_wide_device.hpp.
template <bool kCkpt>
__global__ __launch_bounds__(64 * kWideWaves * kWideMaxWps, 1) void hash_chain_wide_kernel(
    const efes_job* __restrict__ jobs, uint32_t njobs, const Tables* __restrict__ tabs, void* scratch,
    efes_checkpoint* const* __restrict__ ckpt) {
  __shared__ __attribute__((aligned(16))) WideLDS L;
  extern __shared__ __attribute__((aligned(16))) uint8_t chain_wide_xs[];  // blockDim.x x kXStride
  constexpr bool kCopy = false;
  void* const* const dsts = nullptr;
#include "efes_chain_wide_body.inc"
}

hipError_t launch_hash_chain_wide(const efes_job* jobs, uint32_t njobs, efes_checkpoint* const* ckpt, void* scratch,
                                  const Tables* tabs, int cus, hipStream_t s) {
  if (njobs == 0) return hipSuccess;
  const hipError_t e = launch_hash_chain_prep(jobs, njobs, scratch, s);
  if (e != hipSuccess) return e;
  if (ckpt) return launch_wide_walk<hash_chain_wide_kernel<true>>(njobs, cus, s, jobs, njobs, tabs, scratch, ckpt);
  return launch_wide_walk<hash_chain_wide_kernel<false>>(njobs, cus, s, jobs, njobs, tabs, scratch,
                                                         (efes_checkpoint* const*)nullptr);
}

}  // namespace efes
