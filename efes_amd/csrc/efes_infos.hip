// efes_infos.hip -- efes_infos_unmarshal_text and efes_infos_marshal_text: the `.info` texts of an object table
// decoded into its per-object states on the device, and the states encoded back (efes_hash.h "Object infos").  A
// translation unit, and so a code object, of its own, so that the code objects of the other .hip files are the ones
// they were without it.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "efes_infos_rules.hpp"
#include "efes_internal.hpp"

namespace efes {

// ------------------------------------------------------------------ object infos
// Both kernels give a record 32 lanes, so a wavefront holds two records and a workgroup kInfosRecords; the grid is
// sized from n.  Lane l < 26 of a record owns text word l: the 8 characters at text + 208 i + 8 l, one 64-bit load or
// store.  208 = 26 x 8, so the 52 words of a wavefront's two records are contiguous, and so are the 26 state words
// of a record.
//   * infos_unmarshal_kernel: the lane decodes its word (infos_decode_word) into a 32-bit value and a validity bit;
//     the record's verdict is the ballot of those bits masked to the record's half of the wavefront (the six lanes
//     without a text word, and the lanes of a record behind n, vote "valid").  The same lane then stores, at the
//     state word its text word fills (infos_state_word), the value (infos_word_value) or the refusing image's word;
//     lane 25 stores the CRC, lane 26 _pad, lane 27 the status.  Every word of a state is written once, by one lane.
//     The counters: infos_counts_kernel sets counts to {n, 0} in stream order in front; each wavefront counts its
//     invalid records from the ballot, the workgroup adds them up in LDS, and thread 0 of a workgroup that HAS invalid
//     records moves their number from counts[0] to counts[1] with two vector atomics.  A table without a broken text
//     takes no atomic at all.  The first version added both sums in every workgroup: 131 072 workgroups x 2 atomics
//     on two words took 1.6 of the call's 1.6 ms at 1 048 576 records (one word takes about 88 atomics per
//     microsecond), which is why the workgroup also holds 32 records, not 8.
//   * infos_marshal_kernel: the inverse; lane l reads its state word (or the CRC, or nothing for a digest the table
//     does not keep) and stores infos_encode_word of it.
// Every lane checks its record index against n before it loads or stores; no wave waits for another; the only
// atomics are those two on counts[]; no inline assembly.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; profiles/infos/resources.txt):
// no scratch, no spills.
constexpr uint32_t kInfosBlock = 1024;                // lanes of a workgroup
constexpr uint32_t kInfosLanes = 32;                  // lanes of a record
constexpr uint32_t kInfosRecords = kInfosBlock / kInfosLanes;
constexpr uint32_t kInfosWaves = kInfosBlock / 64;
constexpr uint32_t kInfosPadLane = kInfosTextWords, kInfosStatusLane = kInfosTextWords + 1;
static_assert(kInfosStatusLane < kInfosLanes, "a record's 32 lanes hold its 26 text words, _pad and the status");

static inline uint32_t infos_blocks(uint32_t n) { return (n + kInfosRecords - 1) / kInfosRecords; }

__global__ __launch_bounds__(kInfosBlock) void infos_unmarshal_kernel(const uint64_t* __restrict__ text, uint32_t n,
                                                                      uint32_t* __restrict__ sha1, uint32_t* __restrict__ crc32,
                                                                      int32_t* __restrict__ status, uint32_t* __restrict__ counts) {
  __shared__ uint32_t wbad[kInfosWaves];
  const uint32_t l = threadIdx.x & (kInfosLanes - 1u), half = (threadIdx.x >> 5) & 1u, wave = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * kInfosRecords + threadIdx.x / kInfosLanes;
  const bool live = i < n;
  uint32_t value = 0;
  bool ok = true;
  if (live && l < kInfosTextWords) ok = infos_decode_word(text[(size_t)kInfosTextWords * i + l], &value);
  const unsigned long long votes = __ballot(ok);  // of the whole wavefront: no lane has left
  const bool lo_ok = (uint32_t)votes == 0xFFFFFFFFu, hi_ok = (uint32_t)(votes >> 32) == 0xFFFFFFFFu;
  const bool valid = half ? hi_ok : lo_ok;
  if (live) {
    if (l < kInfosShaWords) {
      if (sha1) {
        const uint32_t at = infos_state_word(l);
        sha1[(size_t)kInfosStateWords * i + at] = valid ? infos_word_value(l, value) : infos_refused_word(at);
      }
    } else if (l == kInfosCrcWord) {
      if (crc32) crc32[i] = valid ? value : 0u;
    } else if (l == kInfosPadLane) {
      if (sha1) sha1[(size_t)kInfosStateWords * i + kInfosPadWord] = 0u;
    } else if (l == kInfosStatusLane) {
      if (status) status[i] = valid ? EFES_OK : EFES_ERR_INVALID_DIGEST;
    }
  }
  if (!counts) return;  // uniform
  if ((threadIdx.x & 63u) == 0) {
    // the wavefront's records are 2 * (threadIdx.x / 64) and the next; this lane's own i is the first of them
    const uint32_t have = i < n ? (i + 1 < n ? 2u : 1u) : 0u;
    wbad[wave] = (have > 0 && !lo_ok ? 1u : 0u) + (have > 1 && !hi_ok ? 1u : 0u);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t bad = 0;
#pragma unroll
    for (uint32_t k = 0; k < kInfosWaves; ++k) bad += wbad[k];
    if (bad) {  // counts[0] started at n: bad <= the records of this workgroup, so it never passes below 0
      atomicSub(counts, bad);
      atomicAdd(counts + 1, bad);
    }
  }
}

// counts = {n, 0}: every text valid until infos_unmarshal_kernel finds one that is not.
__global__ void infos_counts_kernel(uint32_t n, uint32_t* __restrict__ counts) {
  if (threadIdx.x == 0) {
    counts[0] = n;
    counts[1] = 0u;
  }
}

__global__ __launch_bounds__(kInfosBlock) void infos_marshal_kernel(const uint32_t* __restrict__ sha1,
                                                                    const uint32_t* __restrict__ crc32, uint32_t n,
                                                                    uint64_t* __restrict__ text) {
  const uint32_t l = threadIdx.x & (kInfosLanes - 1u);
  const uint32_t i = blockIdx.x * kInfosRecords + threadIdx.x / kInfosLanes;
  if (i >= n || l >= kInfosTextWords) return;
  uint32_t v = 0;  // a digest the table does not keep marshals as zeros
  if (l == kInfosCrcWord) {
    if (crc32) v = crc32[i];
  } else if (sha1) {
    v = infos_word_value(l, sha1[(size_t)kInfosStateWords * i + infos_state_word(l)]);
  }
  text[(size_t)kInfosTextWords * i + l] = infos_encode_word(v);
}

hipError_t launch_infos_unmarshal(const efes_infos& in, hipStream_t s) {
  clear_last_error();
  if (in.counts) {
    hipLaunchKernelGGL(infos_counts_kernel, dim3(1), dim3(64), 0, s, in.n, in.counts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (in.n == 0) return hipSuccess;
  hipLaunchKernelGGL(infos_unmarshal_kernel, dim3(infos_blocks(in.n)), dim3(kInfosBlock), 0, s,
                     reinterpret_cast<const uint64_t*>(in.text), in.n, reinterpret_cast<uint32_t*>(in.sha1),
                     reinterpret_cast<uint32_t*>(in.crc32), in.status, in.counts);
  return hipGetLastError();
}

hipError_t launch_infos_marshal(const efes_infos& in, hipStream_t s) {
  if (in.n == 0) return hipSuccess;
  clear_last_error();
  hipLaunchKernelGGL(infos_marshal_kernel, dim3(infos_blocks(in.n)), dim3(kInfosBlock), 0, s,
                     reinterpret_cast<const uint32_t*>(in.sha1), reinterpret_cast<const uint32_t*>(in.crc32), in.n,
                     reinterpret_cast<uint64_t*>(in.text));
  return hipGetLastError();
}

}  // namespace efes
