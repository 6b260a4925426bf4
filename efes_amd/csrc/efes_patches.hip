// efes_patches.hip -- efes_patches_table: the object table of an arrival log of PATCH requests, made on the device
// (efes_hash.h "PATCH logs").  A translation unit, and so a code object, of its own, so that the code objects of the
// other .hip files are the ones they were without it; the scan helper and the digit pass of efes_objects_order.hip
// are restated here for that reason, over 32-bit keys and with the number of passes fixed on the host.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "efes_internal.hpp"
#include "efes_patches_rules.hpp"

namespace efes {

// Stream-ordered launches over the caller's scratch, every grid sized from an element count.  Every lane checks its
// element index against the count before it loads or stores; a key is clamped below nobjects when it is made
// (patch_key); an arrival index from the sort is clamped below npatches before it indexes the log or answers[];
// first[] is clamped to npatches before it bounds a segment; a scatter position is checked against npatches before
// the store.  The only atomics are vector atomics: 32-bit adds in LDS, and on counts[] at most eight per admission
// workgroup that holds a verdict other than ADMITTED.  No wave waits for another; no inline assembly.  Resources
// (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; profiles/patches/resources.txt): no
// scratch, no spills.
constexpr uint32_t kPatchBlock = 1024;  // lanes of a scan or sort workgroup; two scan levels cover kPatchBlock^2
constexpr uint32_t kPatchWaves = kPatchBlock / 64;
constexpr uint32_t kPatchTile = kPatchBlock;  // pairs of one sort workgroup: one per lane
constexpr uint32_t kPatchRadix = 256;
constexpr uint32_t kPatchAdmitBlock = 256;  // objects of one admission workgroup: one per lane
constexpr uint32_t kPatchLane = 64;         // the longest segment one lane walks; a longer one takes the wavefront
static_assert((uint64_t)kPatchRadix * (EFES_OBJECTS_MAX / kPatchTile) <= (uint64_t)kPatchBlock * kPatchBlock,
              "two scan levels cover the digit counts of every tile");

static inline uint32_t patch_blocks(uint32_t n) { return (n + kPatchBlock - 1) / kPatchBlock; }
static inline uint32_t patch_tiles(uint32_t n) { return (n + kPatchTile - 1) / kPatchTile; }

// Sum of v over the workgroup's kPatchBlock lanes, and this lane's exclusive prefix (wsum: kPatchWaves LDS words),
// modulo 2^32: order_block_scan of efes_objects_order.hip.
__device__ uint32_t patch_block_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
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
  for (uint32_t k = 0; k < kPatchWaves; ++k) {
    const uint32_t s = wsum[k];
    if (k < wave) base += s;
    tot += s;
  }
  __syncthreads();  // wsum may be written again
  *total = tot;
  return base + inc - v;
}

#define EFES_PATCH_LAUNCHED()                \
  do {                                       \
    const hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) return e_;         \
  } while (0)

// ------------------------------------------------------------------ the sort
// A stable LSD radix-256 sort of (key = the clamped object, value = the arrival index) from the identity:
//   * patches_keys_kernel (one lane per PATCH) fills buffer 0;
//   * patch_passes(nobjects) digit passes of three launches each, buffer d & 1 to the other one:
//       - patches_count_kernel (one lane per pair, kPatchTile per workgroup): counts[v * tiles + t] = the pairs of
//         tile t with digit value v;
//       - patches_scan_kernel (one lane per count): the exclusive sums within each block of kPatchBlock counts, in
//         place, and each block's sum;
//       - patches_scatter_kernel (grid of the count kernel): the second scan level over the block sums, then every
//         pair goes to (pairs with a smaller digit value) + (pairs of that value in earlier tiles) + (its rank
//         among the pairs of that value in its tile, in index order: whole wavefronts before it by a table in LDS,
//         lanes before it by a match over the wavefront's ballots).  Stable.
struct PatchScratch {
  uint32_t *key[2], *val[2], *counts, *csum;
};
static inline PatchScratch patch_scratch_of(void* scratch, uint32_t npatches) {
  PatchScratch S;
  S.key[0] = static_cast<uint32_t*>(scratch);
  S.key[1] = S.key[0] + npatches;
  S.val[0] = S.key[1] + npatches;
  S.val[1] = S.val[0] + npatches;
  S.counts = S.val[1] + npatches;
  S.csum = S.counts + kPatchRadix * patch_tiles(npatches);
  return S;
}

size_t patches_table_scratch_bytes(uint32_t nobjects, uint32_t npatches) {
  if (nobjects > EFES_OBJECTS_MAX || npatches > EFES_OBJECTS_MAX) return 0;
  const uint32_t ncounts = kPatchRadix * patch_tiles(npatches);
  const size_t words = 4 * (size_t)npatches + ncounts + patch_blocks(ncounts);
  const size_t bytes = (words * 4 + 15) & ~(size_t)15;
  return bytes ? bytes : 16;  // never 0
}

__global__ __launch_bounds__(kPatchBlock) void patches_keys_kernel(const efes_patch* __restrict__ log, uint32_t n, uint32_t m,
                                                                   uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t a = blockIdx.x * kPatchBlock + threadIdx.x;
  if (a < n) {
    key[a] = patch_key(log[a].object, m);
    val[a] = a;
  }
}

__device__ __forceinline__ uint32_t patch_digit(uint32_t key, uint32_t d) { return (key >> (8u * d)) & 0xFFu; }

// The lanes of this wavefront, among those of `valid`, whose digit value equals this lane's.
__device__ __forceinline__ unsigned long long patch_match(uint32_t v, unsigned long long valid) {
  unsigned long long same = valid;
#pragma unroll
  for (uint32_t b = 0; b < 8; ++b) {
    const unsigned long long set = __ballot((v >> b) & 1u);
    same &= ((v >> b) & 1u) ? set : ~set;
  }
  return same;
}

__global__ __launch_bounds__(kPatchBlock) void patches_count_kernel(const uint32_t* __restrict__ key, uint32_t n, uint32_t tiles,
                                                                    uint32_t d, uint32_t* __restrict__ counts) {
  __shared__ uint32_t hist[kPatchRadix];
  if (threadIdx.x < kPatchRadix) hist[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * kPatchTile + threadIdx.x, lane = threadIdx.x & 63u;
  const bool have = i < n;
  const uint32_t v = have ? patch_digit(key[i], d) : 0u;
  const unsigned long long same = patch_match(v, __ballot(have));
  if (have && (same & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&hist[v], (uint32_t)__popcll(same));  // the group's first lane
  __syncthreads();
  if (threadIdx.x < kPatchRadix && blockIdx.x < tiles) counts[threadIdx.x * tiles + blockIdx.x] = hist[threadIdx.x];
}

__global__ __launch_bounds__(kPatchBlock) void patches_scan_kernel(uint32_t* __restrict__ counts, uint32_t ncounts,
                                                                   uint32_t* __restrict__ csum) {
  __shared__ uint32_t wsum[kPatchWaves];
  const uint32_t c = blockIdx.x * kPatchBlock + threadIdx.x;
  uint32_t total;
  const uint32_t excl = patch_block_scan(c < ncounts ? counts[c] : 0u, wsum, &total);
  if (c < ncounts) counts[c] = excl;
  if (threadIdx.x == 0) csum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kPatchBlock) void patches_scatter_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                                      uint32_t* __restrict__ key_to, uint32_t* __restrict__ val_to,
                                                                      uint32_t n, uint32_t tiles, uint32_t d,
                                                                      const uint32_t* __restrict__ counts,
                                                                      const uint32_t* __restrict__ csum) {
  __shared__ uint32_t wsum[kPatchWaves];
  __shared__ uint32_t cpre[kPatchBlock];               // the block sums of the counts' scan, scanned
  __shared__ uint32_t gbase[kPatchRadix];              // where this tile's pairs of each digit value begin
  __shared__ uint32_t wtab[kPatchWaves][kPatchRadix];  // the pairs of each value in each wavefront, then in those before it
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const uint32_t ncounts = kPatchRadix * tiles, cblocks = (ncounts + kPatchBlock - 1) / kPatchBlock;  // <= kPatchBlock
  uint32_t unused;
  cpre[t] = patch_block_scan(t < cblocks ? csum[t] : 0u, wsum, &unused);
  for (uint32_t k = t; k < kPatchWaves * kPatchRadix; k += kPatchBlock) (&wtab[0][0])[k] = 0u;
  __syncthreads();
  if (t < kPatchRadix) {
    const uint32_t c = t * tiles + blockIdx.x;  // < ncounts: blockIdx.x < tiles
    gbase[t] = c < ncounts ? counts[c] + cpre[c / kPatchBlock] : 0u;
  }
  const uint32_t i = blockIdx.x * kPatchTile + t;
  const bool have = i < n;
  uint32_t k = 0u, x = 0u;
  if (have) {
    k = key[i];
    x = val[i];
  }
  const uint32_t v = have ? patch_digit(k, d) : 0u;
  const unsigned long long same = patch_match(v, __ballot(have));
  const uint32_t before = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
  if (have && before == 0u) wtab[wave][v] = (uint32_t)__popcll(same);  // one lane per value and wavefront
  __syncthreads();
  if (t < kPatchRadix) {  // wtab[w][t] = the pairs of value t in the wavefronts before w
    uint32_t at = 0u;
#pragma unroll
    for (uint32_t w = 0; w < kPatchWaves; ++w) {
      const uint32_t c = wtab[w][t];
      wtab[w][t] = at;
      at += c;
    }
  }
  __syncthreads();
  if (have) {
    const uint32_t to = gbase[v] + wtab[wave][v] + before;
    if (to < n) {  // always, for counts that this launch's own count pass made
      key_to[to] = k;
      val_to[to] = x;
    }
  }
}

// ------------------------------------------------------------------ the boundaries
// first[i] = the first slot whose key is not below i: a lower bound in the sorted keys, one lane per boundary;
// first[0] = 0 and first[nobjects] = npatches whatever the keys hold (every key is below nobjects).
__global__ __launch_bounds__(kPatchBlock) void patches_first_kernel(const uint32_t* __restrict__ key, uint32_t n, uint32_t m,
                                                                    uint32_t* __restrict__ first) {
  const uint32_t i = blockIdx.x * kPatchBlock + threadIdx.x;
  if (i > m) return;
  uint32_t lo = 0, hi = n;
  if (i == 0) hi = 0;
  if (i == m) lo = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (key[mid] < i)
      lo = mid + 1;
    else
      hi = mid;
  }
  first[i] = lo;
}

// counts = {npatches, 0, 0, 0, 0}: every PATCH ADMITTED until the admission pass finds one that is not.
__global__ void patches_counts_kernel(uint32_t n, uint32_t* __restrict__ counts) {
  if (blockIdx.x == 0 && threadIdx.x < kPatchVerdicts) counts[threadIdx.x] = threadIdx.x == 0 ? n : 0u;
}

// ------------------------------------------------------------------ the admission
// One lane per object, kPatchAdmitBlock per workgroup.  A lane walks its own segment of at most kPatchLane slots
// with patch_step.  Behind that the wavefront takes its longer segments one after the other: 64 slots per step, the
// records loaded side by side, then resolved RUN BY RUN rather than one by one.  After an admitted PATCH cur is
// always that PATCH's file_offset + length (a restart has file_offset 0), so the PATCHes behind it whose
// file_offset equals their predecessor's end are admitted as well, up to the first that is DONE: one ballot finds
// the next PATCH that fits cur, one the end of its run.  A well-formed log resolves in one run per step; patch_step
// is what each run restates, and the twin's outputs are the check.  Every lane then stores its slot's extent, its
// PATCH's answer (scattered to arrival order) and patch_of; the object's lane its record and, for a restarted
// upload, its fresh states.
struct PatchRecord {
  efes_patch p;
  uint32_t arrival;
};

__device__ __forceinline__ PatchRecord patch_load(const efes_patch* __restrict__ log, const uint32_t* __restrict__ val, uint32_t n,
                                                  uint32_t k) {
  PatchRecord r;
  const uint32_t a = val[k];
  r.arrival = a < n ? a : n - 1;  // n > 0: a slot exists
  r.p = log[r.arrival];
  return r;
}

struct PatchOut {
  efes_extent* extents;
  efes_patch_answer* answers;
  uint32_t* patch_of;
};

__device__ __forceinline__ void patch_store(const PatchOut& out, uint32_t k, const PatchRecord& r, uint32_t verdict, uint64_t answer) {
  const bool hashed = patch_hashed(verdict);
  efes_extent e;
  e.offset = hashed ? r.p.data_offset : 0ull;
  e.length = hashed ? r.p.length : 0ull;
  out.extents[k] = e;
  if (out.answers) {
    efes_patch_answer w;
    w.offset = answer;
    w.verdict = verdict;
    w.slot = k;
    out.answers[r.arrival] = w;
  }
  if (out.patch_of) out.patch_of[k] = r.arrival;
}

// Bits [from, to) of a 64-bit mask; from <= to <= 64.
__device__ __forceinline__ unsigned long long patch_bits(uint32_t from, uint32_t to) {
  const unsigned long long below_to = to >= 64u ? ~0ull : (1ull << to) - 1ull;
  const unsigned long long below_from = from >= 64u ? ~0ull : (1ull << from) - 1ull;
  return below_to & ~below_from;
}

__global__ __launch_bounds__(kPatchAdmitBlock) void patches_admit_kernel(const efes_patches in, const uint32_t* __restrict__ val) {
  __shared__ uint32_t moved[kPatchVerdicts];  // the workgroup's PATCHes per verdict other than ADMITTED
  const uint32_t m = in.nobjects, n = in.npatches;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * kPatchAdmitBlock + threadIdx.x;
  if (threadIdx.x < kPatchVerdicts) moved[threadIdx.x] = 0u;
  __syncthreads();
  const PatchOut out = {in.extents, in.answers, in.patch_of};
  const bool mine = i < m;
  uint32_t begin = 0, end = 0;
  PatchAuto a = patch_begin(0ull);
  if (mine) {
    const uint32_t f0 = in.first[i], f1 = in.first[i + 1];
    begin = f0 < n ? f0 : n;
    end = f1 < n ? f1 : n;
    if (end < begin) end = begin;
    a = patch_begin(in.offsets ? in.offsets[i] : 0ull);
  }
  uint32_t conflicts = 0, deferred = 0, done = 0, invalid = 0;
  const bool wide = end - begin > kPatchLane;
  if (!wide) {
    for (uint32_t k = begin; k < end; ++k) {
      const PatchRecord r = patch_load(in.log, val, n, k);
      uint64_t answer = 0;
      const uint32_t verdict =
          r.p.object < m ? patch_step(a, r.p.file_offset, r.p.length, r.p.file_length, &answer) : (uint32_t)EFES_PATCH_INVALID;
      patch_store(out, k, r, verdict, answer);
      conflicts += verdict == EFES_PATCH_CONFLICT;
      deferred += verdict == EFES_PATCH_DEFERRED;
      done += verdict == EFES_PATCH_DONE;
      invalid += verdict == EFES_PATCH_INVALID;
    }
  }
  unsigned long long todo = __ballot(wide);
  while (todo) {  // uniform: the wavefront's long segments, one after the other
    const uint32_t owner = (uint32_t)__ffsll((long long)todo) - 1u;
    todo &= todo - 1ull;
    const uint32_t b = __shfl(begin, owner, 64), e = __shfl(end, owner, 64);
    uint64_t cur = __shfl((unsigned long long)a.cur, owner, 64);  // uniform from here on
    uint32_t flags = 0, admitted = 0;
    for (uint32_t base = b; base < e; base += 64u) {
      const uint32_t k = base + lane;
      const bool have = k < e;
      PatchRecord r;
      r.arrival = 0;
      r.p.data_offset = r.p.length = r.p.file_offset = r.p.file_length = 0ull;
      r.p.object = 0xFFFFFFFFu;
      r.p._reserved = 0;
      if (have) r = patch_load(in.log, val, n, k);
      const bool valid = have && r.p.object < m;
      const uint64_t my_end = r.p.file_offset + r.p.length;  // cur behind this PATCH if it is admitted
      const uint64_t prev_end = __shfl_up((unsigned long long)my_end, 1, 64);
      const unsigned long long valids = __ballot(valid);
      const unsigned long long zeros = __ballot(valid && r.p.file_offset == 0);
      const unsigned long long links = __ballot(valid && lane > 0 && r.p.file_offset != 0 && r.p.file_offset == prev_end) & (valids << 1);
      const unsigned long long dones = __ballot(valid && my_end == r.p.file_length);
      uint32_t verdict = EFES_PATCH_INVALID;
      uint64_t answer = 0;
      uint32_t pos = 0;
      while (pos < 64u) {  // uniform
        const unsigned long long rest = ~0ull << pos;
        if (flags & kPatchClosedBits) {  // everything behind is deferred
          if (valids & rest) flags |= EFES_PATCH_OBJ_DEFERRED;
          if (valid && lane >= pos) {
            verdict = EFES_PATCH_DEFERRED;
            answer = cur;
          }
          break;
        }
        const unsigned long long fit = __ballot(valid && (r.p.file_offset == 0 || r.p.file_offset == cur)) & rest;
        const uint32_t at = fit ? (uint32_t)__ffsll((long long)fit) - 1u : 64u;
        if (valid && lane >= pos && lane < at) {
          verdict = EFES_PATCH_CONFLICT;
          answer = cur;
        }
        if (at == 64u) break;
        if ((zeros >> at) & 1ull) {
          if (admitted) {  // a restart behind admitted bytes closes the object; the branch above defers from `at` on
            flags |= EFES_PATCH_OBJ_DEFERRED;
            pos = at;
            continue;
          }
          flags |= EFES_PATCH_OBJ_RESTARTED;
        }
        const unsigned long long unlinked = ~links & ((~0ull << at) << 1);
        uint32_t stop = unlinked ? (uint32_t)__ffsll((long long)unlinked) - 1u : 64u;  // the run is [at, stop)
        const unsigned long long ends = dones & patch_bits(at, stop);
        uint32_t last_done = 64u;
        if (ends) {
          last_done = (uint32_t)__ffsll((long long)ends) - 1u;
          stop = last_done + 1u;
          flags |= EFES_PATCH_OBJ_DONE;
        }
        if (lane >= at && lane < stop) {
          verdict = lane == last_done ? EFES_PATCH_DONE : EFES_PATCH_ADMITTED;
          answer = my_end;
        }
        admitted += stop - at;
        cur = __shfl((unsigned long long)my_end, stop - 1u, 64);
        pos = stop;
      }
      if (have) {
        patch_store(out, k, r, verdict, answer);
        conflicts += verdict == EFES_PATCH_CONFLICT;
        deferred += verdict == EFES_PATCH_DEFERRED;
        done += verdict == EFES_PATCH_DONE;
        invalid += verdict == EFES_PATCH_INVALID;
      }
    }
    if (lane == owner) {
      a.cur = cur;
      a.flags = flags;
      a.admitted = admitted;
    }
  }
  if (mine) {
    if (in.objects) {
      efes_patch_object o;
      o.offset = a.cur;
      o.flags = a.flags;
      o.admitted = a.admitted;
      in.objects[i] = o;
    }
    if (a.flags & EFES_PATCH_OBJ_RESTARTED) {
      if (in.sha1) {
        uint32_t* s = reinterpret_cast<uint32_t*>(in.sha1 + i);
#pragma unroll
        for (uint32_t w = 0; w < kPatchStateWords; ++w) s[w] = patch_fresh_word(w);
      }
      if (in.crc32) in.crc32[i].crc = 0u;
    }
  }
  if (!in.counts) return;  // uniform
  if (__ballot((conflicts | deferred | done | invalid) != 0u)) {  // uniform over the wavefront
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      conflicts += __shfl_xor(conflicts, off, 64);
      deferred += __shfl_xor(deferred, off, 64);
      done += __shfl_xor(done, off, 64);
      invalid += __shfl_xor(invalid, off, 64);
    }
    if (lane == 0) {
      if (conflicts) atomicAdd(&moved[EFES_PATCH_CONFLICT], conflicts);
      if (deferred) atomicAdd(&moved[EFES_PATCH_DEFERRED], deferred);
      if (done) atomicAdd(&moved[EFES_PATCH_DONE], done);
      if (invalid) atomicAdd(&moved[EFES_PATCH_INVALID], invalid);
    }
  }
  __syncthreads();
  if (threadIdx.x >= 1 && threadIdx.x < kPatchVerdicts) {
    const uint32_t c = moved[threadIdx.x];
    if (c) {  // counts[0] started at npatches: c <= the PATCHes of this workgroup, so it never passes below 0
      atomicSub(in.counts, c);
      atomicAdd(in.counts + threadIdx.x, c);
    }
  }
}

hipError_t launch_patches_table(const efes_patches& in, void* scratch, hipStream_t s) {
  const uint32_t m = in.nobjects, n = in.npatches;
  clear_last_error();
  hipError_t e;
  if (in.counts) {
    hipLaunchKernelGGL(patches_counts_kernel, dim3(1), dim3(64), 0, s, n, in.counts);
    EFES_PATCH_LAUNCHED();
  }
  const uint32_t* val = nullptr;
  if (n == 0) {  // every segment is empty: the admission pass only writes the object records
    e = hipMemsetAsync(in.first, 0, ((size_t)m + 1) * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (!in.objects || m == 0) return hipSuccess;
  } else {
    const PatchScratch S = patch_scratch_of(scratch, n);
    const uint32_t tiles = patch_tiles(n), ncounts = kPatchRadix * tiles, passes = patch_passes(m);
    hipLaunchKernelGGL(patches_keys_kernel, dim3(patch_blocks(n)), dim3(kPatchBlock), 0, s, in.log, n, m, S.key[0], S.val[0]);
    EFES_PATCH_LAUNCHED();
    for (uint32_t d = 0; d < passes; ++d) {
      const uint32_t src = d & 1u, dst = src ^ 1u;
      hipLaunchKernelGGL(patches_count_kernel, dim3(tiles), dim3(kPatchBlock), 0, s, (const uint32_t*)S.key[src], n, tiles, d, S.counts);
      EFES_PATCH_LAUNCHED();
      hipLaunchKernelGGL(patches_scan_kernel, dim3(patch_blocks(ncounts)), dim3(kPatchBlock), 0, s, S.counts, ncounts, S.csum);
      EFES_PATCH_LAUNCHED();
      hipLaunchKernelGGL(patches_scatter_kernel, dim3(tiles), dim3(kPatchBlock), 0, s, (const uint32_t*)S.key[src],
                         (const uint32_t*)S.val[src], S.key[dst], S.val[dst], n, tiles, d, (const uint32_t*)S.counts,
                         (const uint32_t*)S.csum);
      EFES_PATCH_LAUNCHED();
    }
    hipLaunchKernelGGL(patches_first_kernel, dim3(patch_blocks(m + 1)), dim3(kPatchBlock), 0, s, (const uint32_t*)S.key[passes & 1u], n, m,
                       in.first);
    EFES_PATCH_LAUNCHED();
    val = S.val[passes & 1u];
  }
  hipLaunchKernelGGL(patches_admit_kernel, dim3((m + kPatchAdmitBlock - 1) / kPatchAdmitBlock), dim3(kPatchAdmitBlock), 0, s, in, val);
  return hipGetLastError();
}

}  // namespace efes
