// efes_kernels.hip -- MI355X (gfx950) kernels for efes' per-chunk SHA-1 + CRC-32/IEEE.
//
// Semantics: every efes_job is one `Write(p)` of the reference's
//   sha1digest.Write  (/root/reference/sha1.go:58-79)  and
//   crc32digest.Write (/root/reference/crc32.go:76-86 -> slicingUpdate :153-169)
// into a device-resident state, optionally followed by Sum (sha1.go:82-120 checkSum,
// crc32.go:88-93).  Go panics (nx > 64 at Write, d.nx != 0 in checkSum) become
// EFES_ERR_STATE.  The tail buffer x is updated byte-for-byte as Go does, stale bytes
// included, so MarshalText (sha1_efes.go:25-38) of a device state equals Go's.
//
// Two kernel shapes (DESIGN_NOTES.md):
//   DEEP: one chain wavefront per job.  SHA-1 is a strict chain of 64-byte compressions, so a
//         job's speed is one wave's issue rate.  A producer wave on the same SIMD loads 64
//         consecutive blocks (4 KiB, coalesced), computes their CRC-32 partials (combined by a
//         6-level GF(2) shift tree) and expands each block's schedule W[i]+K[i]; the chain wave
//         copies its lane's block W+K from LDS into registers, the 80-round chain of block i
//         runs in lane i (5 VALU per round) and the chaining value steps to lane i+1 by DPP:
//         405 chain VALU + 5 DPP moves per block.
//   GROUPn: 64/n jobs per wavefront (n lanes each), the DEEP chain shared by the jobs.
//   WIDE: one lane per job (64 jobs per wave), schedule inline, CRC fused per lane.
//         Throughput shape for many concurrent jobs.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "efes_internal.hpp"
#include "sha1_device.hpp"
#include "efes_wide_device.hpp"

#ifdef EFES_CHECKED
// Debug build only (tools/debug_checked.py): every data load is range-checked against the
// job's [p, p+plen); a violation is printed and redirected to p so the kernel cannot fault.
#include <stdio.h>
#define EFES_RANGE(ptr, nbytes, lo, len, tag)                                                               \
  (((const uint8_t*)(ptr) < (const uint8_t*)(lo) ||                                                          \
    (const uint8_t*)(ptr) + (nbytes) > (const uint8_t*)(lo) + (len))                                         \
       ? (printf("EFES_CHECKED %s: ptr=%p n=%d lo=%p len=%llu blk=%d thr=%d\n", tag, (const void*)(ptr),        \
                 (int)(nbytes), (const void*)(lo), (unsigned long long)(len), (int)blockIdx.x, (int)threadIdx.x), \
          (decltype(ptr))(lo))                                                                              \
       : (ptr))
#else
#define EFES_RANGE(ptr, nbytes, lo, len, tag) (ptr)
#endif

namespace efes {

// ================================================================== DEEP kernel

constexpr int kGroupMaxJobs = 16;  // jobs per wave in the grouped DEEP kernel (G = 4)

// One job's running state between the phases of a DEEP wave (head -> bulk -> rest),
// parked in LDS while the wave's other jobs run their phases.
struct DeepMsg {
  uint32_t h[5];
  uint32_t crc_raw;
  const uint8_t* q;  // first bulk byte (p + pos)
  uint64_t pos;      // bytes consumed by the head
  uint64_t nbulk;    // whole blocks after the head
  uint64_t done;     // bulk blocks already hashed by the joint phase
  int64_t nx_new;
  uint32_t live;     // 0: no job, or Go panicked in the head
  uint32_t joint;    // takes part in the grouped kernel's current joint round
};

struct DeepLDS {
  Tables tab;                                    // 36 KiB
  PosTables pos;                                 // 64 KiB, follows tab (same order as in HBM)
  uint8_t xs[kDeepWaves][kGroupMaxJobs][64];     // each job's tail buffer x (sha1.go:31)
  uint8_t fin[kDeepWaves][192];                  // padding assembly for checkSum
  DeepMsg msg[kDeepWaves][kGroupMaxJobs];
};
static_assert(offsetof(DeepLDS, pos) == sizeof(Tables), "DeepLDS copies Tables+PosTables in one sweep");

struct DeepJob {
  const uint8_t* p;
  uint64_t plen;
  efes_sha1_state* st;
  efes_crc32_state* cs;
  uint8_t* sum;
  int32_t* status;
  uint32_t flags;
};

// Bulk blocks q[0 .. 64*nbulk) of one job by one wave alone (the one-job path, used for a
// grouped wave's left-over blocks through deep_rest).  The DEEP kernel proper splits this same super-step between a producer and a chain wave
// (pipe_produce / pipe_consume below).  Per super-step of up to 64 blocks (4 KiB, one coalesced
// load per lane, prefetched a super-step ahead): lane off+i holds block i, computes its raw
// CRC-32 (slicing-by-8, LDS tables) and expands its schedule W[t]+K[t] into its own 80 VGPRs.
// The block CRCs are merged by a 6-level GF(2) shift tree.  Then the wave runs the SHA-1
// chain 64 times with the SAME register names: in iteration i only lane off+i computes the
// real compression (its W+K registers hold block i) and the other lanes compute garbage in
// the same instructions, so the chain reads W+K straight from registers -- no LDS traffic.
// The chaining value moves from lane off+i to lane off+i+1 by DPP wave_shr:1 (5 v_mov_dpp
// per block).  Measured against W+K read back from LDS by ds_read_b128: 48.1 vs 52.7 ms per
// 1024 x 4 MiB (DESIGN_NOTES.md §4).
template <bool kAligned16>
__device__ void deep_bulk(const Tables& T, int lane, const uint8_t* q, uint64_t nbulk, bool do_sha, bool do_crc,
                          uint32_t (&h)[5], uint32_t& crc_raw) {
  uint32_t le[16];
  // Blocks are right-aligned in the lanes (lane 64-nb+i holds block i) so that the zero
  // CRCs of idle lanes lead the tree, and the last block of every super-step is in lane 63.
  uint64_t b0 = 0;
  int nb = (int)(nbulk < 64 ? nbulk : 64);
  {
    const int bi = lane - (64 - nb);
#pragma unroll
    for (int k = 0; k < 16; ++k) le[k] = 0;
    if (bi >= 0) load_block_le<kAligned16>(EFES_RANGE(q + 64 * (uint64_t)bi, 64, q, 64 * nbulk, "deep-bulk0"), le);
  }
  while (b0 < nbulk) {
    if (do_crc) {
      uint32_t r = crc_words_raw(T.slice8, 0u, le);  // raw CRC of this lane's block, register 0
#pragma unroll
      for (int k = 0; k < 6; ++k) {  // crc(A||B) = shift(crc(A), |B|) ^ crc(B), |B| = 64<<k bytes
        const uint32_t o = __shfl_xor(r, 1 << k);
        const bool right = (lane >> k) & 1;
        r = crc_shift(T.shift[k], right ? o : r) ^ (right ? r : o);
      }
      if (nb == 64) {
        crc_raw = crc_shift(T.shift[6], crc_raw);
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k)
          if ((nb >> k) & 1) crc_raw = crc_shift(T.shift[k], crc_raw);
      }
      crc_raw ^= r;
    }
    uint32_t x[80];  // this lane's block: W[t] + K[t], t = 0..79
    if (do_sha) {
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = bswap(le[k]);
      expand_wk(w, x);
    }
    // Prefetch the next super-step's blocks; they land while the chain runs.
    const uint64_t b1 = b0 + (uint64_t)nb;
    const int nb1 = (int)((nbulk - b1) < 64 ? (nbulk - b1) : 64);
    if (b1 < nbulk) {
      const int bj = lane - (64 - nb1);
#pragma unroll
      for (int k = 0; k < 16; ++k) le[k] = 0;
      if (bj >= 0) load_block_le<kAligned16>(EFES_RANGE(q + 64 * (b1 + (uint64_t)bj), 64, q, 64 * nbulk, "deep-bulk1"), le);
    }
    if (do_sha) {
      uint32_t hv[5] = {h[0], h[1], h[2], h[3], h[4]}, hs[5];
      auto block = [&]() {
        chain_block(hv, x, hs);  // sha1.go:193-197 folded in
#pragma unroll
        for (int k = 1; k < 6; ++k) hv[k % 5] = (uint32_t)__builtin_amdgcn_mov_dpp((int)hs[k % 5], 0x138, 0xf, 0xf, true);  // wave_shr:1, h0 (round 79's v_add3) last
      };
      const int nbu = (int)uniform32((uint32_t)nb);
      int j = 0;
      for (; j + 2 <= nbu; j += 2) { block(); block(); }  // unrolled by two: half the loop overhead
      if (j < nbu) block();
#pragma unroll
      for (int k = 0; k < 5; ++k) h[k] = (uint32_t)__builtin_amdgcn_readlane((int)hs[k], 63);
    }
    b0 = b1;
    nb = nb1;
  }
}

// Head of one Write (sha1.go:58-69): load the state, complete a pending x[:nx].  Returns the
// job's running state; live == 0 when Go would panic (status already written).
__device__ DeepMsg deep_head(const Tables& T, int lane, const DeepJob& J, uint8_t* xs) {
  const bool do_sha = J.st != nullptr, do_crc = J.cs != nullptr;
  DeepMsg M{};
  uint32_t (&h)[5] = M.h;
  int64_t nx = 0;
  const bool init = (J.flags & EFES_JOB_INIT) != 0;
  if (do_sha && init) {  // NewSha1(): zero value + Reset (sha1.go:36-52)
    h[0] = kIV0; h[1] = kIV1; h[2] = kIV2; h[3] = kIV3; h[4] = kIV4;
    if (lane < 16) reinterpret_cast<uint32_t*>(xs)[lane] = 0u;
  } else if (do_sha) {
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = uniform32(J.st->h[k]);
    nx = (int64_t)uniform64((uint64_t)J.st->nx);
    if (lane < 16) reinterpret_cast<uint32_t*>(xs)[lane] = reinterpret_cast<const uint32_t*>(J.st->x)[lane];
  }
  uint32_t crc_raw = do_crc ? (init ? 0xFFFFFFFFu : ~uniform32(J.cs->crc)) : 0u;

  if (do_sha && nx > 64) {  // Go: copy(d.x[d.nx:], p) panics (sha1.go:62)
    if (lane == 0 && J.status) *J.status = EFES_ERR_STATE;
    return M;
  }
  const uint8_t* p = J.p;
  const uint64_t plen = J.plen;
  wave_lds_sync();

  // ---- complete the pending block x[:nx] (sha1.go:61-69)
  uint64_t pos = 0;
  int64_t nx_new = nx;
  if (do_sha && nx > 0) {
    const uint32_t room = (uint32_t)(64 - nx);
    const uint32_t nh = plen < room ? (uint32_t)plen : room;
    if ((uint32_t)lane < nh) xs[nx + lane] = ldg_u8(EFES_RANGE(p + lane, 1, p, plen, "deep-head"));
    wave_lds_sync();
    if ((uint32_t)nx + nh == 64) {
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = be_word_lds(xs, k);
      compress_inline(h, w);
      nx_new = 0;
    } else {
      nx_new = nx + nh;
    }
    pos = nh;
  }
  if (do_crc)
    for (uint64_t i = 0; i < pos; ++i) crc_raw = crc_byte(T.slice8[0], crc_raw, ldg_u8(EFES_RANGE(p + i, 1, p, plen, "deep-crchead")));
  M.crc_raw = crc_raw;
  M.q = p + pos;
  M.pos = pos;
  M.nbulk = (plen - pos) >> 6;
  M.done = 0;
  M.nx_new = nx_new;
  M.live = 1;
  return M;
}

// The rest of one Write after the head: bulk blocks [M.done, M.nbulk) (sha1.go:70-74), the
// tail (:75-77), Sum (:82-120) on a copy, and the write-back of state, crc, sum and status.
// kBulk = false: the caller has hashed every bulk block (M.done == M.nbulk) and T may hold only
// the slicing-by-8 table (FED kernel).
template <bool kBulk = true>
__device__ void deep_rest(const Tables& T, int lane, const DeepJob& J, uint8_t* xs, uint8_t* fb, DeepMsg M) {
  const bool do_sha = J.st != nullptr, do_crc = J.cs != nullptr;
  const bool fin = (J.flags & EFES_JOB_FINALIZE) != 0;
  int32_t status = EFES_OK;
  uint32_t (&h)[5] = M.h;
  uint32_t crc_raw = M.crc_raw;
  int64_t nx_new = M.nx_new;
  const uint8_t* p = J.p;
  const uint64_t plen = J.plen;
  const uint64_t pos = M.pos, nbulk = M.nbulk;
  uint64_t len = do_sha && !(J.flags & EFES_JOB_INIT) ? uniform64(J.st->len) : 0;

  // ---- bulk whole blocks not hashed yet (sha1.go:70-74)
  if (kBulk && nbulk > M.done) {
    const uint8_t* q = M.q + 64 * M.done;
    if ((reinterpret_cast<uintptr_t>(q) & 15) == 0)
      deep_bulk<true>(T, lane, q, nbulk - M.done, do_sha, do_crc, h, crc_raw);
    else
      deep_bulk<false>(T, lane, q, nbulk - M.done, do_sha, do_crc, h, crc_raw);
  }

  // ---- tail (sha1.go:75-77): x[:r] = rest; x[r:] keeps stale bytes
  const uint64_t tpos = pos + (nbulk << 6);
  const uint32_t r = (uint32_t)(plen - tpos);
  if (do_crc)
    for (uint32_t i = 0; i < r; ++i) crc_raw = crc_byte(T.slice8[0], crc_raw, ldg_u8(EFES_RANGE(p + tpos + i, 1, p, plen, "deep-crctail")));
  if (do_sha && r > 0) {
    if ((uint32_t)lane < r) xs[lane] = ldg_u8(EFES_RANGE(p + tpos + lane, 1, p, plen, "deep-tail"));
    nx_new = r;
  }
  wave_lds_sync();
  len += plen;  // sha1.go:60

  // ---- Sum (sha1.go:89-120) on a copy of the state
  uint32_t dig[5] = {0, 0, 0, 0, 0};
  bool have_sum = false;
  if (fin && do_sha) {
    const uint32_t nxf = nx_new > 0 ? (uint32_t)nx_new : 0u;  // Write skips a negative nx (sha1.go:61)
    const uint32_t lm = (uint32_t)(len & 63);
    const uint32_t padlen = lm < 56 ? 56 - lm : 120 - lm;     // sha1.go:94-98
    const uint32_t T = nxf + padlen + 8;
    if (T & 63) {
      status = EFES_ERR_STATE;  // sha1.go:107-109 panic("d.nx != 0")
    } else {
      const uint64_t bits = len << 3;
      for (uint32_t i = lane; i < T; i += 64) {
        uint32_t b;
        if (i < nxf) b = xs[i];
        else if (i == nxf) b = 0x80;
        else if (i >= T - 8) b = (uint32_t)(bits >> (56 - 8 * (i - (T - 8)))) & 0xffu;
        else b = 0;
        fb[i] = (uint8_t)b;
      }
      wave_lds_sync();
      uint32_t hf[5] = {h[0], h[1], h[2], h[3], h[4]};
      for (uint32_t blk = 0; blk < T / 64; ++blk) {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = be_word_lds(fb + 64 * blk, k);
        compress_inline(hf, w);
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) dig[k] = hf[k];
      have_sum = true;
    }
  }

  // ---- write back (a Sum-only job leaves the states alone: Go's Sum works on a copy)
  const bool keep = (J.flags & EFES_JOB_SUM_ONLY) != 0;
  if (do_sha && !keep) {
    if (lane < 5) {
      uint32_t v = h[0];
#pragma unroll
      for (int k = 1; k < 5; ++k) v = lane == k ? h[k] : v;
      J.st->h[lane] = v;
    }
    if (lane < 16) reinterpret_cast<uint32_t*>(J.st->x)[lane] = reinterpret_cast<const uint32_t*>(xs)[lane];
    if (lane == 0) {
      J.st->nx = nx_new;
      J.st->len = len;
    }
  }
  if (do_crc && !keep && lane == 0) J.cs->crc = ~crc_raw;
  if (fin && J.sum && lane < 6) {
    uint32_t v;
    if (lane < 5) {
      v = dig[0];
#pragma unroll
      for (int k = 1; k < 5; ++k) v = lane == k ? dig[k] : v;
      v = have_sum ? v : 0u;
    } else {
      v = do_crc ? ~crc_raw : 0u;
    }
    reinterpret_cast<uint32_t*>(J.sum)[lane] = bswap(v);  // big-endian, as Sum appends
  }
  if (lane == 0 && J.status) *J.status = status;
}

// Job j's descriptor as wave-uniform values.
__device__ __forceinline__ DeepJob load_job(const efes_job* __restrict__ jobs, uint32_t j, int lane) {
  const efes_job* jb = jobs + j;
  DeepJob J;
  J.p = reinterpret_cast<const uint8_t*>(uniform64(reinterpret_cast<uint64_t>(jb->data)));
  J.plen = uniform64(jb->length);
  J.st = reinterpret_cast<efes_sha1_state*>(uniform64(reinterpret_cast<uint64_t>(jb->sha1)));
  J.cs = reinterpret_cast<efes_crc32_state*>(uniform64(reinterpret_cast<uint64_t>(jb->crc32)));
  J.sum = reinterpret_cast<uint8_t*>(uniform64(reinterpret_cast<uint64_t>(jb->sum)));
  J.status = reinterpret_cast<int32_t*>(uniform64(reinterpret_cast<uint64_t>(jb->status)));
  J.flags = uniform32(jb->flags);
#ifdef EFES_CHECKED
  if (lane == 0)
    printf("EFES_CHECKED job %u p=%p len=%llu st=%p cs=%p sum=%p status=%p flags=%u\n", j, (const void*)J.p,
           (unsigned long long)J.plen, (void*)J.st, (void*)J.cs, (void*)J.sum, (void*)J.status, J.flags);
#else
  (void)lane;
#endif
  return J;
}

// DeepMsg field read back from LDS as a wave-uniform value.
__device__ __forceinline__ DeepMsg uniform_msg(const DeepMsg& s) {
  DeepMsg M;
#pragma unroll
  for (int k = 0; k < 5; ++k) M.h[k] = uniform32(s.h[k]);
  M.crc_raw = uniform32(s.crc_raw);
  M.q = reinterpret_cast<const uint8_t*>(uniform64(reinterpret_cast<uint64_t>(s.q)));
  M.pos = uniform64(s.pos);
  M.nbulk = uniform64(s.nbulk);
  M.done = uniform64(s.done);
  M.nx_new = (int64_t)uniform64((uint64_t)s.nx_new);
  M.live = uniform32(s.live);
  M.joint = uniform32(s.joint);
  return M;
}

// ================================================================== DEEP kernel, producer/consumer
// Workgroup = 4 chain waves + 4 producer waves; wave w+4 always lands on the same SIMD as wave
// w (tools/microbench/mb_placement.hip), so each SIMD hosts one job's chain and its producer.
// The producer does everything of a super-step that is not the chain -- the coalesced load of
// 64 blocks, their CRC-32 and shift tree, the W+K expansion -- and hands W+K over through LDS
// (20 ds_write_b128 per lane); the chain wave (s_setprio 3) only copies its block's 80 words
// into registers (20 ds_read_b128 per lane per super-step) and runs the 64 chains.  The chain
// wave's instruction stream is then 405 + 5 per block plus ~30 per 64 blocks.
constexpr int kPipeJobs = 4;  // jobs per workgroup (one per SIMD)

struct PipeSlot {  // one job's hand-over area
  uint4 wk[20][64];  // [word quad][lane]: lane l's block W+K[4q..4q+3] -- conflict-free b128 access
  DeepMsg msg;       // the head's result (chain -> producer), then the final CRC (producer -> chain)
  int started;       // chain -> producer: msg holds the head's result
  int ready;         // producer -> chain: super-steps whose W+K has been written
  int taken;         // chain -> producer: super-steps whose W+K the chain has copied out
  int crc_done;      // producer -> chain: msg.crc_raw is the CRC after the bulk
};

struct PipeLDS {
  Tables tab;                                // 36 KiB
  PipeSlot slot[kPipeJobs];                  // 4 x 20 KiB
  uint8_t xs[kPipeJobs][64];
  uint8_t fin[kPipeJobs][192];
};

__device__ __forceinline__ int lds_acquire(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void lds_release(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <int kSleep>
__device__ __forceinline__ void wait_at_least(const int* p, int v) {
  while (lds_acquire(p) < v) __builtin_amdgcn_s_sleep(kSleep);
}

// Producer side of deep_bulk: super-steps of up to 64 blocks, right-aligned in the lanes.
template <bool kAligned16>
__device__ void pipe_produce(const Tables& T, PipeSlot& P, int lane, const uint8_t* q, uint64_t nbulk, bool do_sha,
                             bool do_crc, uint32_t& crc_raw) {
  uint32_t le[16];
  uint64_t b0 = 0;
  int nb = (int)(nbulk < 64 ? nbulk : 64);
  {
    const int bi = lane - (64 - nb);
#pragma unroll
    for (int k = 0; k < 16; ++k) le[k] = 0;
    if (bi >= 0) load_block_le<kAligned16>(EFES_RANGE(q + 64 * (uint64_t)bi, 64, q, 64 * nbulk, "pipe-bulk0"), le);
  }
  for (int step = 0; b0 < nbulk; ++step) {
    if (do_crc) {
      uint32_t r = crc_words_raw(T.slice8, 0u, le);
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const uint32_t o = __shfl_xor(r, 1 << k);
        const bool right = (lane >> k) & 1;
        r = crc_shift(T.shift[k], right ? o : r) ^ (right ? r : o);
      }
      if (nb == 64) {
        crc_raw = crc_shift(T.shift[6], crc_raw);
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k)
          if ((nb >> k) & 1) crc_raw = crc_shift(T.shift[k], crc_raw);
      }
      crc_raw ^= r;
    }
    uint32_t x[80];
    if (do_sha) {
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = bswap(le[k]);
      expand_wk(w, x);
    }
    const uint64_t b1 = b0 + (uint64_t)nb;
    const int nb1 = (int)((nbulk - b1) < 64 ? (nbulk - b1) : 64);
    if (b1 < nbulk) {
      const int bj = lane - (64 - nb1);
#pragma unroll
      for (int k = 0; k < 16; ++k) le[k] = 0;
      if (bj >= 0) load_block_le<kAligned16>(EFES_RANGE(q + 64 * (b1 + (uint64_t)bj), 64, q, 64 * nbulk, "pipe-bulk1"), le);
    }
    if (do_sha) {
      wait_at_least<8>(&P.taken, step);  // the chain has copied super-step step-1 out
#pragma unroll
      for (int k = 0; k < 20; ++k) P.wk[k][lane] = make_uint4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
      lds_release(&P.ready, step + 1);
    }
    b0 = b1;
    nb = nb1;
  }
}

// Chain side: per super-step, copy this lane's block W+K out of LDS and run the nb chains.
__device__ void pipe_consume(PipeSlot& P, int lane, uint64_t nbulk, uint32_t (&h)[5]) {
  uint64_t b0 = 0;
  for (int step = 0; b0 < nbulk; ++step) {
    const int nb = (int)((nbulk - b0) < 64 ? (nbulk - b0) : 64);
    wait_at_least<1>(&P.ready, step + 1);
    uint32_t x[80];
#pragma unroll
    for (int k = 0; k < 20; ++k) {
      const uint4 v = P.wk[k][lane];
      x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
    }
    lds_release(&P.taken, step + 1);  // (release: the reads above complete first)
    uint32_t hv[5] = {h[0], h[1], h[2], h[3], h[4]}, hs[5];
    auto block = [&]() {
      chain_block(hv, x, hs);  // sha1.go:193-197 folded in
#pragma unroll
      for (int k = 1; k < 6; ++k) hv[k % 5] = (uint32_t)__builtin_amdgcn_mov_dpp((int)hs[k % 5], 0x138, 0xf, 0xf, true);  // wave_shr:1, h0 (round 79's v_add3) last
    };
    const int nbu = (int)uniform32((uint32_t)nb);
    int j = 0;
    for (; j + 2 <= nbu; j += 2) { block(); block(); }
    if (j < nbu) block();
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = (uint32_t)__builtin_amdgcn_readlane((int)hs[k], 63);
    b0 += (uint64_t)nb;
  }
}

__global__ __launch_bounds__(128 * kPipeJobs, 1) void deep_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                                  const Tables* __restrict__ tabs) {
  __shared__ __attribute__((aligned(16))) PipeLDS L;
  {
    const uint4* src = reinterpret_cast<const uint4*>(tabs);
    uint4* dst = reinterpret_cast<uint4*>(&L.tab);
    for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 16); i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x < kPipeJobs) {
      PipeSlot& P = L.slot[threadIdx.x];
      P.started = P.ready = P.taken = P.crc_done = 0;
    }
  }
  __syncthreads();
  const int wave = (int)uniform32(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int w = wave & (kPipeJobs - 1);
  const uint32_t j = blockIdx.x * kPipeJobs + (uint32_t)w;
  if (j >= njobs) return;
  PipeSlot& P = L.slot[w];
  const DeepJob J = load_job(jobs, j, lane);
  const bool do_sha = J.st != nullptr, do_crc = J.cs != nullptr;
  if (wave < kPipeJobs) {  // ---- chain wave
    __builtin_amdgcn_s_setprio(3);
    DeepMsg M = deep_head(L.tab, lane, J, L.xs[w]);
    if (lane == 0) P.msg = M;
    lds_release(&P.started, 1);
    if (!M.live) return;
    if (do_sha) pipe_consume(P, lane, M.nbulk, M.h);
    wait_at_least<1>(&P.crc_done, 1);
    M.crc_raw = uniform32(P.msg.crc_raw);
    M.done = M.nbulk;
    deep_rest(L.tab, lane, J, L.xs[w], L.fin[w], M);
  } else {  // ---- producer wave
    wait_at_least<4>(&P.started, 1);
    const DeepMsg M = uniform_msg(P.msg);
    if (!M.live) return;
    uint32_t crc_raw = M.crc_raw;
    if (M.nbulk) {
      if ((reinterpret_cast<uintptr_t>(M.q) & 15) == 0)
        pipe_produce<true>(L.tab, P, lane, M.q, M.nbulk, do_sha, do_crc, crc_raw);
      else
        pipe_produce<false>(L.tab, P, lane, M.q, M.nbulk, do_sha, do_crc, crc_raw);
    }
    if (lane == 0) P.msg.crc_raw = crc_raw;
    lds_release(&P.crc_done, 1);
  }
}

// The value of the last lane of each group of G lanes, in every lane of the group: a job's
// chaining value after a super-step, back to all its lanes.  G = 4 is one quad: a DPP
// quad_perm [3,3,3,3] move (no LDS round trip on the chain's critical path); wider groups use
// ds_bpermute.
template <int G>
__device__ __forceinline__ uint32_t group_last(uint32_t v, int lane) {
  if constexpr (G == 4) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xFF, 0xf, 0xf, true);
  return (uint32_t)__shfl((int)v, lane | (G - 1));
}

// ================================================================== grouped DEEP kernel
// k = 64/G jobs per wave, G lanes (= G consecutive blocks per super-step) per job.  For
// batches with more long jobs than SIMDs: the chain instructions are shared by the k jobs
// (lane m*G+i runs block i of job m), so a super-step of 410 G + ~700 instructions advances
// k jobs by G blocks each: (410 G + ~700)/64 instructions per block of issue work (DEEP: 422)
// at a per-job latency of 410 + ~700/G per block (WIDE: 740 at a slower issue rate).
// DESIGN_NOTES.md §4 "grouped DEEP".
//
// Phases per wave: the head of every job (sequential, state parked in LDS); joint rounds in
// which the jobs with >= G bulk blocks left advance together; then, per job, the rest
// (left-over bulk blocks through deep_bulk, tail, Sum, write-back).  Jobs are expected
// longest-first (efes_plan_batch) so the jobs of a wave have similar lengths.
// Raw CRC (register 0) of one 64-byte block: the XOR of 64 independent position-table lookups
// (PosTables), in four accumulation chains.
__device__ __forceinline__ uint32_t crc_block_pos(const uint32_t (&pos)[64][256], const uint32_t (&le)[16]) {
  uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int w = 0; w < 16; ++w) {
    const uint32_t v = le[w];
    const uint32_t x = __builtin_amdgcn_bitop3_b32(pos[4 * w][v & 0xffu], pos[4 * w + 1][(v >> 8) & 0xffu],
                                                   pos[4 * w + 2][(v >> 16) & 0xffu], 0x96);
    acc[w & 3] = __builtin_amdgcn_bitop3_b32(acc[w & 3], x, pos[4 * w + 3][v >> 24], 0x96);
  }
  return __builtin_amdgcn_bitop3_b32(acc[0], acc[1], acc[2], 0x96) ^ acc[3];
}

// kSha / kCrc are wave-uniform (any joining job needs the hash): with both, the CRC lookups and
// the schedule expansion share one basic block, so the lookups' latency hides behind VALU work.
// kUser: the kernel that calls it (0 group_kernel, 1 hash_chain_group_kernel, 2 hash_chain_group_ckpt_kernel), so that each has an
// instantiation of its own, with one call site, and compiles as if the other did not exist.
template <int G, bool kAligned16, bool kSha, bool kCrc, int kUser = 0>
__device__ void group_bulk(const Tables& T, const PosTables& P, int lane, DeepMsg* msgs, uint64_t S) {
  constexpr int kLG = G == 4 ? 2 : G == 8 ? 3 : G == 16 ? 4 : 5;
  static_assert((1 << kLG) == G, "G must be 4, 8, 16 or 32");
  const int m = lane / G, i = lane % G;
  const DeepMsg& M = msgs[m];
  const bool live = M.live != 0 && M.joint != 0;
  const uint8_t* q = M.q + 64 * M.done;
  uint32_t hv[5] = {M.h[0], M.h[1], M.h[2], M.h[3], M.h[4]}, hs[5] = {0, 0, 0, 0, 0};
  uint32_t crc_raw = M.crc_raw;
  // One super-step: CRC + schedule of this lane's block `cur`, the prefetch of the next
  // super-step's block into `nxt` (exec-masked: a lane of a job outside this round loads
  // nothing; zeroed first so the compiler keeps the prefetch a whole chain ahead), the chain.
  auto super_step = [&](const uint32_t (&cur)[16], uint32_t (&nxt)[16], uint64_t st) {
    if constexpr (kCrc) {
      uint32_t r = crc_block_pos(P.pos, cur);  // raw CRC of this lane's block, register 0
#pragma unroll
      for (int k = 0; k < kLG; ++k) {  // crc(A||B) = shift(crc(A), |B|) ^ crc(B) within the job's G lanes
        const uint32_t o = __shfl_xor(r, 1 << k);
        const bool right = (lane >> k) & 1;
        r = crc_shift(T.shift[k], right ? o : r) ^ (right ? r : o);
      }
      crc_raw = crc_shift(T.shift[kLG], crc_raw) ^ r;  // running crc advanced over G*64 bytes
    }
    uint32_t x[80];
    if constexpr (kSha) {
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = bswap(cur[k]);
      expand_wk(w, x);
    }
    if (st + 1 < S) {
#pragma unroll
      for (int k = 0; k < 16; ++k) nxt[k] = 0;
      if (live) load_block_le<kAligned16>(q + 64 * ((st + 1) * G + (uint64_t)i), nxt);
    }
    if constexpr (kSha) {
      auto block = [&]() {
        chain_block(hv, x, hs);  // real in lane m*G+j of every job m at iteration j
#pragma unroll
        for (int k = 1; k < 6; ++k) hv[k % 5] = (uint32_t)__builtin_amdgcn_mov_dpp((int)hs[k % 5], 0x138, 0xf, 0xf, true);  // wave_shr:1, h0 (round 79's v_add3) last
      };
#pragma unroll
      for (int j = 0; j < G; j += 2) { block(); block(); }
      // the job's chaining value is in its last lane: back to all G lanes (its first one needs it)
#pragma unroll
      for (int k = 0; k < 5; ++k) hv[k] = group_last<G>(hs[k], lane);
    }
  };
  uint32_t A[16], B[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) A[k] = 0;
  if (live) load_block_le<kAligned16>(q + 64 * (uint64_t)i, A);
  for (uint64_t st = 0; st < S; st += 2) {  // two buffers, unrolled by two: no register copies of the prefetch
    super_step(A, B, st);
    if (st + 1 >= S) break;
    super_step(B, A, st + 1);
  }
  wave_lds_sync();
  if (live && i == 0) {  // joint jobs only
    DeepMsg& W = msgs[m];
#pragma unroll
    for (int k = 0; k < 5; ++k) W.h[k] = kSha ? hv[k] : W.h[k];
    W.crc_raw = crc_raw;
    W.done += S * G;
  }
  wave_lds_sync();
}

template <int G, bool kAligned16, int kUser = 0>
__device__ void group_bulk_any(const Tables& T, const PosTables& P, int lane, DeepMsg* msgs, uint64_t S, bool any_sha,
                               bool any_crc) {
  if (any_sha && any_crc) group_bulk<G, kAligned16, true, true, kUser>(T, P, lane, msgs, S);
  else if (any_sha) group_bulk<G, kAligned16, true, false, kUser>(T, P, lane, msgs, S);
  else group_bulk<G, kAligned16, false, true, kUser>(T, P, lane, msgs, S);
}


template <int G>
__global__ __launch_bounds__(64 * kDeepWaves, 1) void group_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                                   const Tables* __restrict__ tabs) {
  constexpr int kJobs = 64 / G;
  static_assert(kJobs <= kGroupMaxJobs, "LDS holds kGroupMaxJobs jobs per wave");
  __shared__ __attribute__((aligned(16))) DeepLDS L;
  {
    const uint4* src = reinterpret_cast<const uint4*>(tabs);  // Tables then PosTables
    uint4* dst = reinterpret_cast<uint4*>(&L.tab);
    for (int i = threadIdx.x; i < (int)((sizeof(Tables) + sizeof(PosTables)) / 16); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int wave = (int)uniform32(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const uint32_t j0 = (blockIdx.x * kDeepWaves + (uint32_t)wave) * kJobs;
  if (j0 >= njobs) return;
  DeepMsg* msgs = L.msg[wave];

  // ---- heads (state parked in LDS)
  for (int m = 0; m < kJobs; ++m) {
    const uint32_t j = j0 + (uint32_t)m;
    DeepMsg M{};
    if (j < njobs) M = deep_head(L.tab, lane, load_job(jobs, j, lane), L.xs[wave][m]);
    wave_lds_sync();
    if (lane == 0) msgs[m] = M;
  }
  wave_lds_sync();

  // ---- joint rounds: while two or more jobs have >= G bulk blocks left, they advance together
  // by S*G blocks, S = the smallest of their floor(left/G) (so a wave lasts as long as its
  // longest job, whatever the mix of lengths); a job left alone finishes on the one-job path
  // (422 instructions per block instead of (410 G + ~700)/G).
  for (int round = 0; round < kJobs; ++round) {
    uint64_t S = ~0ull;
    int joiners = 0;
    bool any_sha = false, any_crc = false, all16 = true;
    for (int m = 0; m < kJobs; ++m) {
      const DeepMsg M = uniform_msg(msgs[m]);
      const uint64_t left = M.live ? (M.nbulk - M.done) / G : 0;
      if (left == 0) continue;
      ++joiners;
      S = left < S ? left : S;
      const DeepJob J = load_job(jobs, j0 + (uint32_t)m, lane);
      any_sha |= J.st != nullptr;
      any_crc |= J.cs != nullptr;
      all16 &= (reinterpret_cast<uintptr_t>(M.q + 64 * M.done) & 15) == 0;
    }
    if (joiners < 2) break;
    for (int m = 0; m < kJobs; ++m) {
      const DeepMsg M = uniform_msg(msgs[m]);
      if (lane == 0) msgs[m].joint = M.live && (M.nbulk - M.done) / G > 0 ? 1u : 0u;
    }
    wave_lds_sync();
    if (all16) group_bulk_any<G, true>(L.tab, L.pos, lane, msgs, S, any_sha, any_crc);
    else group_bulk_any<G, false>(L.tab, L.pos, lane, msgs, S, any_sha, any_crc);
  }

  // ---- per job: left-over blocks, tail, Sum, write-back
  for (int m = 0; m < kJobs; ++m) {
    const uint32_t j = j0 + (uint32_t)m;
    if (j >= njobs) break;
    const DeepMsg M = uniform_msg(msgs[m]);
    if (!M.live) continue;
    const DeepJob J = load_job(jobs, j, lane);
    deep_rest(L.tab, lane, J, L.xs[wave][m], L.fin[wave], M);
  }
}

// ================================================================== FED kernel: grouped DEEP fed from other SIMDs
// The grouped kernel's chain wave spends (410 G + ~665) instructions per super-step: the chain
// plus the loads, CRC and W+K expansion of its 64 blocks, all on one SIMD, so a job's latency is
// 410 + 665/G per block (GROUP4: 577).  Here a workgroup owns its CU (its LDS fills the CU) and
// splits that work across the CU's four SIMDs (one wave each): C chain waves holding 64/G jobs of
// G lanes each, and 4 - C producer waves.  Per super-step of a chain wave, its producer loads the
// 64 blocks (G consecutive blocks of each job, coalesced, prefetched a super-step ahead), computes
// their CRC-32 (position tables: 64 independent lookups per block, the G-lane shift tree, the fold
// into each job's running CRC) and the W+K expansion, and hands W+K over through LDS as the DEEP
// kernel does (20 ds_write_b128 per lane).  The chain wave copies its lane's 80 words out
// (20 ds_read_b128) and runs G chains: 410 + ~50/G instructions per block, DEEP's per-job latency.
// A producer serves its chain waves round-robin, polling their slots (measured: one item, i.e.
// one chain super-step, costs the producer ~3.9k cycles against the chain's ~6.9k at G = 4).
// Heads, left-over blocks (< G per job), tails and Sums run on the chain waves.
//   FED4 = <G 4, 2 chain waves + 2 producers>: 32 jobs per CU.
template <int G, int C>
struct FedCfg {
  static constexpr int kJobs = 64 / G;  // jobs per chain wave
  static constexpr int kProducers = 4 - C;
  static constexpr int kLG = G == 4 ? 2 : G == 8 ? 3 : 0;
  static_assert(kLG > 0 && C >= 1 && C <= 3, "G in {4, 8}, 1..3 chain waves");
};

// FED4E: the producer hands over the 16 message words W[0..15] (big-endian); the chain wave
// expands W[16..79] and adds K.  (Round 2 measured handing over more of the schedule: no gain.)
constexpr int kFedHand = 16;

struct FedSlot {
  uint4 wk[20][64];   // [word quad][lane], as PipeSlot
  uint64_t S;         // super-steps of the posted round
  uint32_t flags;     // bit 0: some joint job hashes SHA-1, bit 1: CRC-32, bit 2: all blocks 16-B aligned
  uint32_t req;       // chain -> producer: rounds posted
  uint32_t fin;       // chain -> producer: no more rounds
  uint32_t ready;     // producer -> chain: super-steps whose W+K is in wk (running count)
  uint32_t taken;     // chain -> producer: super-steps copied out of wk
  uint32_t crc_done;  // producer -> chain: rounds whose CRCs are back in the job's DeepMsg
};

// The LDS copy of the tables: the slicing-by-8 table and shift levels 0..3 (the tree and fold for
// G <= 8) -- a prefix of Tables, so deep_head / deep_rest<false> can take it as one -- and the
// position tables for the producer's CRC.
constexpr int kFedShift = 4;
struct FedTables {
  uint32_t slice8[8][256];
  uint32_t shift[kFedShift][4][256];
};
static_assert(offsetof(Tables, shift) == offsetof(FedTables, shift), "FedTables is a prefix of Tables");

template <int G, int C>
struct FedLDS {
  static constexpr int kJobs = FedCfg<G, C>::kJobs;
  FedTables tab;                // 24 KiB
  PosTables pos;                // 64 KiB
  FedSlot slot[C];              // 20 KiB each
  DeepMsg msg[C][kJobs];
  uint8_t xs[C][kJobs][64];
  uint8_t fin[C][192];
};

// Counters run modulo 2^32: "a has reached b".
__device__ __forceinline__ bool reached(uint32_t a, uint32_t b) { return (int32_t)(a - b) >= 0; }
__device__ __forceinline__ uint32_t lds_acq32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// Release store issued HERE: the scheduling barrier keeps the compiler from sinking it below the
// (fully unrolled) work that follows, which would hold the other side up for that long.
__device__ __forceinline__ void lds_rel32(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  __builtin_amdgcn_sched_barrier(0);
}

// One lane's block of a fed super-step (zeros for a lane whose job sits the round out).
__device__ __forceinline__ void fed_load(const uint8_t* src, bool live, bool a16, uint32_t (&le)[16]) {
#pragma unroll
  for (int k = 0; k < 16; ++k) le[k] = 0;
  if (live) {
    if (a16) load_block_le<true>(src, le);
    else load_block_le<false>(src, le);
  }
}

// Producer-side state of one chain wave's current round.
struct FedFeed {
  const uint8_t* q;  // this lane's job: first byte of the round (M.q + 64 * (M.done + i))
  uint64_t S, st;    // super-steps of the round, produced so far
  uint32_t gstep;    // W+K super-steps handed to this chain wave, all rounds
  uint32_t round;    // rounds served
  uint32_t crc;      // this lane's job's running raw CRC
  uint32_t flags;
  bool live, active, done;
  uint32_t pre[16];  // the next super-step's block, in flight
};

template <int G, int C>
__device__ __forceinline__ void fed_start(FedLDS<G, C>& L, int c, int lane, FedFeed& F) {
  FedSlot& P = L.slot[c];
  F.S = uniform64(P.S);
  F.flags = uniform32(P.flags);
  const int m = lane / G, i = lane % G;
  const DeepMsg& M = L.msg[c][m];
  F.live = M.live != 0 && M.joint != 0;
  F.q = M.q + 64 * (M.done + (uint64_t)i);
  F.crc = M.crc_raw;
  F.st = 0;
  F.active = true;
  fed_load(F.q, F.live, (F.flags & 4u) != 0, F.pre);
}

// Produce super-step F.st of chain wave c into its (free) slot.  X: the chain wave expands the
// schedule itself, the producer hands over only the 16 message words (big-endian).
template <int G, int C, bool X>
__device__ __forceinline__ void fed_produce(FedLDS<G, C>& L, int c, int lane, FedFeed& F) {
  constexpr int kLG = FedCfg<G, C>::kLG;
  FedSlot& P = L.slot[c];
  const bool do_sha = (F.flags & 1u) != 0, do_crc = (F.flags & 2u) != 0, a16 = (F.flags & 4u) != 0;
  uint32_t cur[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) cur[k] = F.pre[k];
  if (F.st + 1 < F.S) fed_load(F.q + 64 * G * (F.st + 1), F.live, a16, F.pre);
  if (do_crc) {
    uint32_t r = crc_block_pos(L.pos.pos, cur);  // raw CRC of this lane's block (independent lookups)
#pragma unroll
    for (int k = 0; k < kLG; ++k) {  // the job's G blocks: crc(A||B) = shift(crc(A), |B|) ^ crc(B)
      const uint32_t o = __shfl_xor(r, 1 << k);
      const bool right = (lane >> k) & 1;
      r = crc_shift(L.tab.shift[k], right ? o : r) ^ (right ? r : o);
    }
    F.crc = crc_shift(L.tab.shift[kLG], F.crc) ^ r;  // running CRC advanced over G * 64 bytes
  }
  if (do_sha) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) w[k] = bswap(cur[k]);
    if constexpr (X) {  // the first kFedHand raw schedule words; the chain wave expands the rest
      uint32_t r[kFedHand];
      expand_raw<kFedHand>(w, r);
#pragma unroll
      for (int k = 0; k < kFedHand / 4; ++k) P.wk[k][lane] = make_uint4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
    } else {
      uint32_t x[80];
      expand_wk(w, x);
#pragma unroll
      for (int k = 0; k < 20; ++k) P.wk[k][lane] = make_uint4(x[4 * k], x[4 * k + 1], x[4 * k + 2], x[4 * k + 3]);
    }
    lds_rel32(&P.ready, F.gstep + 1);
    ++F.gstep;  // counts handed-over super-steps only, as the chain's copy-outs do
  }
  if (++F.st == F.S) {  // round done: CRCs back to the jobs' messages
    const int m = lane / G;
    if (F.live && (lane % G) == 0 && do_crc) L.msg[c][m].crc_raw = F.crc;
    ++F.round;
    lds_rel32(&P.crc_done, F.round);
    F.active = false;
  }
}

// Producer p serves chain waves p, p + producers, ... (those of the C that exist: nchains).
template <int G, int C, bool X>
__device__ void fed_producer(FedLDS<G, C>& L, int lane, int p, uint32_t nchains) {
  constexpr int kP = FedCfg<G, C>::kProducers;
  FedFeed F[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    F[c].gstep = 0;
    F[c].round = 0;
    F[c].active = false;
    F[c].done = c % kP != p || (uint32_t)c >= nchains;
  }
  for (;;) {
    bool all_done = true, did = false;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (F[c].done) continue;
      all_done = false;
      FedSlot& P = L.slot[c];
      if (!F[c].active) {
        if (!reached(F[c].round, lds_acq32(&P.req))) {
          fed_start(L, c, lane, F[c]);
        } else {
          if (lds_acq32(&P.fin)) F[c].done = true;
          continue;
        }
      }
      if ((F[c].flags & 1u) && !reached(lds_acq32(&P.taken), F[c].gstep)) continue;  // slot still in use
      fed_produce<G, C, X>(L, c, lane, F[c]);
      did = true;
    }
    if (all_done) break;
    if (!did) __builtin_amdgcn_s_sleep(1);
  }
}

// Chain side of one round: S super-steps of G blocks for every joint job of the wave.
template <int G, bool X>
__device__ void fed_consume(FedSlot& P, int lane, const DeepMsg* msgs, uint64_t S, uint32_t& gstep, uint32_t (&hv)[5]) {
  const DeepMsg& M = msgs[lane / G];
#pragma unroll
  for (int k = 0; k < 5; ++k) hv[k] = M.h[k];
  uint32_t hs[5] = {0, 0, 0, 0, 0};
  for (uint64_t st = 0; st < S; ++st) {
    while (!reached(lds_acq32(&P.ready), gstep + 1)) __builtin_amdgcn_s_sleep(1);
    uint32_t x[80];
    if constexpr (X) {
      uint32_t w[kFedHand];
#pragma unroll
      for (int k = 0; k < kFedHand / 4; ++k) {
        const uint4 v = P.wk[k][lane];
        w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
      }
      lds_rel32(&P.taken, gstep + 1);  // the producer may overwrite the slot now
      expand_wk_from<kFedHand>(w, x);
    } else {
#pragma unroll
      for (int k = 0; k < 20; ++k) {
        const uint4 v = P.wk[k][lane];
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
      }
      lds_rel32(&P.taken, gstep + 1);  // the producer may overwrite the slot now
    }
    ++gstep;
    auto block = [&]() {
      chain_block(hv, x, hs);  // real in lane m*G+j of every job m at iteration j
#pragma unroll
      for (int k = 1; k < 6; ++k) hv[k % 5] = (uint32_t)__builtin_amdgcn_mov_dpp((int)hs[k % 5], 0x138, 0xf, 0xf, true);  // wave_shr:1, h0 (round 79's v_add3) last
    };
#pragma unroll
    for (int j = 0; j < G; ++j) block();
#pragma unroll
    for (int k = 0; k < 5; ++k) hv[k] = group_last<G>(hs[k], lane);
  }
}

template <int G, int C, bool X>
__global__ __launch_bounds__(256, 1) void fed_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                     const Tables* __restrict__ tabs) {
  constexpr int kJobs = FedCfg<G, C>::kJobs;
  __shared__ __attribute__((aligned(16))) FedLDS<G, C> L;
  static_assert(sizeof(FedLDS<G, C>) <= 160 * 1024, "one FED workgroup per CU");
  {
    const uint4* src = reinterpret_cast<const uint4*>(tabs);  // Tables, then PosTables (efes_ctx_create)
    uint4* dst = reinterpret_cast<uint4*>(&L.tab);
    for (int i = threadIdx.x; i < (int)(sizeof(FedTables) / 16); i += blockDim.x) dst[i] = src[i];
    const uint4* psrc = reinterpret_cast<const uint4*>(tabs + 1);
    uint4* pdst = reinterpret_cast<uint4*>(&L.pos);
    for (int i = threadIdx.x; i < (int)(sizeof(PosTables) / 16); i += blockDim.x) pdst[i] = psrc[i];
    if (threadIdx.x < C) {
      FedSlot& P = L.slot[threadIdx.x];
      P.req = P.fin = P.ready = P.taken = P.crc_done = 0;
    }
  }
  __syncthreads();
  const int wave = (int)uniform32(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const uint32_t base = blockIdx.x * (uint32_t)(C * kJobs);
  if (wave >= C) {  // ---- producer (a SIMD of its own)
    const uint32_t left = njobs - base;  // base < njobs for every launched workgroup
    fed_producer<G, C, X>(L, lane, wave - C, (left + kJobs - 1) / kJobs);
    return;
  }
  // ---- chain wave
  __builtin_amdgcn_s_setprio(3);
  const uint32_t j0 = base + (uint32_t)wave * kJobs;
  if (j0 >= njobs) return;  // no producer waits for this chain wave (nchains above)
  FedSlot& P = L.slot[wave];
  DeepMsg* msgs = L.msg[wave];
  const Tables& T = reinterpret_cast<const Tables&>(L.tab);  // slice8 only (deep_head, deep_rest<false>)
  for (int m = 0; m < kJobs; ++m) {  // heads (state parked in LDS)
    const uint32_t j = j0 + (uint32_t)m;
    DeepMsg M{};
    if (j < njobs) M = deep_head(T, lane, load_job(jobs, j, lane), L.xs[wave][m]);
    wave_lds_sync();
    if (lane == 0) msgs[m] = M;
  }
  wave_lds_sync();
  // Joint rounds as in group_kernel, but down to a single job: a lone job still runs at the fed
  // chain's latency, and afterwards every job has fewer than G bulk blocks left.
  uint32_t gstep = 0;
  for (uint32_t round = 0; round < (uint32_t)kJobs; ++round) {
    uint64_t S = ~0ull;
    int joiners = 0;
    bool any_sha = false, any_crc = false, all16 = true;
    for (int m = 0; m < kJobs; ++m) {
      const DeepMsg M = uniform_msg(msgs[m]);
      const uint64_t left = M.live ? (M.nbulk - M.done) / G : 0;
      if (left == 0) continue;
      ++joiners;
      S = left < S ? left : S;
      const DeepJob J = load_job(jobs, j0 + (uint32_t)m, lane);
      any_sha |= J.st != nullptr;
      any_crc |= J.cs != nullptr;
      all16 &= (reinterpret_cast<uintptr_t>(M.q + 64 * M.done) & 15) == 0;
    }
    if (joiners == 0) break;
    for (int m = 0; m < kJobs; ++m) {
      const DeepMsg M = uniform_msg(msgs[m]);
      if (lane == 0) msgs[m].joint = M.live && (M.nbulk - M.done) / G > 0 ? 1u : 0u;
    }
    if (lane == 0) {
      P.S = S;
      P.flags = (any_sha ? 1u : 0u) | (any_crc ? 2u : 0u) | (all16 ? 4u : 0u);
    }
    lds_rel32(&P.req, round + 1);  // release: the messages and S above are visible first
    uint32_t hv[5] = {0, 0, 0, 0, 0};
    if (any_sha) fed_consume<G, X>(P, lane, msgs, S, gstep, hv);
    while (!reached(lds_acq32(&P.crc_done), round + 1)) __builtin_amdgcn_s_sleep(1);
    const int m = lane / G;
    const bool joint = msgs[m].joint != 0;
    wave_lds_sync();
    if (joint && (lane % G) == 0) {
      DeepMsg& W = msgs[m];
#pragma unroll
      for (int k = 0; k < 5; ++k) W.h[k] = any_sha ? hv[k] : W.h[k];
      W.done += S * G;
    }
    wave_lds_sync();
  }
  lds_rel32(&P.fin, 1);
  for (int m = 0; m < kJobs; ++m) {  // per job: the < G left-over blocks, tail, Sum, write-back
    const uint32_t j = j0 + (uint32_t)m;
    if (j >= njobs) break;
    DeepMsg M = uniform_msg(msgs[m]);
    if (!M.live) continue;
    const DeepJob J = load_job(jobs, j, lane);
    for (; M.done < M.nbulk; ++M.done) {  // one block at a time, the same in every lane
      uint32_t le[16];
      load_block_le<false>(M.q + 64 * M.done, le);
      if (J.cs) M.crc_raw = crc_words_raw(T.slice8, M.crc_raw, le);
      if (J.st) {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = bswap(le[k]);
        compress_inline(M.h, w);
      }
    }
    deep_rest<false>(T, lane, J, L.xs[wave][m], L.fin[wave], M);
  }
}

// ================================================================== WIDE kernel
// One lane per job.  Per-lane tail buffers live in LDS with a 68-byte stride (17 dwords:
// lanes touching the same byte index hit different banks).
//
// A workgroup holds every wave a SIMD will run in the launch: 4 x wps waves (wps = waves per SIMD,
// 1..3; wave w runs on SIMD w % 4), one workgroup per CU.  The SIMD issues from the oldest ready
// wave first, so of wps waves with equally long messages the oldest ran at nearly a lone wave's
// rate and ended first, and the last one ran alone -- at a lone wave's ~5.1 cycles per VALU
// instead of 4 -- for the last ~30 % of the launch (per-wave timeline, profiles/r03_wide_timeline:
// the SIMD busy 62 of 72.5 ms).  So the waves of a SIMD publish their progress in LDS and, once per
// loop iteration, the furthest behind takes the top priority and the furthest ahead the lowest
// (s_setprio): they advance together and end together.


__global__ __launch_bounds__(64 * kWideWaves * kWideMaxWps, 1) void wide_kernel(const efes_job* __restrict__ jobs,
                                                                                uint32_t njobs,
                                                                                const Tables* __restrict__ tabs) {
  __shared__ __attribute__((aligned(16))) WideLDS L;
  extern __shared__ __attribute__((aligned(16))) uint8_t wide_xs[];  // blockDim.x x kXStride (launch_wide)
  {
    const uint4* src = wide_tab_src(tabs);
    uint4* dst = reinterpret_cast<uint4*>(L.crc);
    for (int i = threadIdx.x; i < (int)(sizeof(L.crc) / 16); i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x < kWideWaves * kWideMaxWps) L.prog[threadIdx.x] = 0;
  }
  __syncthreads();
  const uint32_t wv = threadIdx.x / 64, nwv = blockDim.x / 64;
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = j < njobs;
  const efes_job jb = live ? jobs[j] : efes_job{};
  const uint8_t* p = reinterpret_cast<const uint8_t*>(jb.data);
  const uint64_t plen = jb.length;
  efes_sha1_state* st = jb.sha1;
  efes_crc32_state* cs = jb.crc32;
  const bool do_sha = live && st != nullptr, do_crc = live && cs != nullptr;
  const bool fin = live && (jb.flags & EFES_JOB_FINALIZE) != 0;
  uint8_t* xl = wide_xs + (size_t)threadIdx.x * kXStride;
  int32_t status = EFES_OK;

  uint32_t h[5] = {0, 0, 0, 0, 0};
  int64_t nx = 0;
  uint64_t len = 0;
  const bool init = live && (jb.flags & EFES_JOB_INIT) != 0;
  if (do_sha && init) {  // NewSha1() (sha1.go:36-52)
    h[0] = kIV0; h[1] = kIV1; h[2] = kIV2; h[3] = kIV3; h[4] = kIV4;
#pragma unroll
    for (int k = 0; k < 64; ++k) xl[k] = 0;
  } else if (do_sha) {
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = st->h[k];
    nx = st->nx;
    len = st->len;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t v = reinterpret_cast<const uint32_t*>(st->x)[k];
      xl[4 * k] = (uint8_t)v; xl[4 * k + 1] = (uint8_t)(v >> 8); xl[4 * k + 2] = (uint8_t)(v >> 16); xl[4 * k + 3] = (uint8_t)(v >> 24);
    }
  }
  uint32_t crc_raw = do_crc ? (init ? 0xFFFFFFFFu : ~cs->crc) : 0u;
  const bool bad = do_sha && nx > 64;  // sha1.go:62 panic
  const bool go = live && !bad;

  // ---- head
  uint64_t pos = 0;
  int64_t nx_new = nx;
  if (go && do_sha && nx > 0) {
    const uint32_t room = (uint32_t)(64 - nx);
    const uint32_t nh = plen < room ? (uint32_t)plen : room;
    for (uint32_t i = 0; i < nh; ++i) xl[nx + i] = ldg_u8(p + i);
    if ((uint32_t)nx + nh == 64) {
      uint32_t w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = be_word_lds(xl, k);
      compress_inline(h, w);
      nx_new = 0;
    } else {
      nx_new = nx + nh;
    }
    pos = nh;
  }
  if (go && do_crc)
    for (uint64_t i = 0; i < pos; ++i) crc_raw = crc_byte(wide_t0(L), crc_raw, ldg_u8(p + i));

  // ---- bulk: lanes iterate their own block counts (masked when done)
  const uint8_t* q = p + pos;
  const uint64_t nbulk = go ? (plen - pos) >> 6 : 0;
  const bool all16 = __all(!go || (reinterpret_cast<uintptr_t>(q) & 15) == 0);
  const bool any_sha = __any(do_sha), any_crc = __any(do_crc);  // wave-uniform
  const uint64_t nmax = wave_max64(nbulk);
  // the shortest message over ALL lanes (a lane without a job has nbulk 0: no uniform phase)
  const uint64_t nmin = wave_min64(nbulk, true);
  const uint8_t* dummy = reinterpret_cast<const uint8_t*>(tabs);  // 36 KiB of valid device memory
  if (all16) wide_bulk_any<true>(q, nbulk, nmin, nmax, dummy, any_sha, any_crc, L.crc, h, crc_raw, L.prog, wv, nwv);
  else wide_bulk_any<false>(q, nbulk, nmin, nmax, dummy, any_sha, any_crc, L.crc, h, crc_raw, L.prog, wv, nwv);
  if ((threadIdx.x & 63) == 0) __atomic_store_n(&L.prog[wv], 0xffffffffu, __ATOMIC_RELAXED);  // done: never the slowest

  // ---- tail
  const uint64_t tpos = pos + (nbulk << 6);
  const uint32_t r = go ? (uint32_t)(plen - tpos) : 0u;
  if (do_crc)
    for (uint32_t i = 0; i < r; ++i) crc_raw = crc_byte(wide_t0(L), crc_raw, ldg_u8(p + tpos + i));
  if (do_sha && r > 0) {
    for (uint32_t i = 0; i < r; ++i) xl[i] = ldg_u8(p + tpos + i);
    nx_new = r;
  }
  len += go ? plen : 0;

  // ---- Sum
  uint32_t dig[5] = {0, 0, 0, 0, 0};
  if (go && fin && do_sha) {
    const uint32_t nxf = nx_new > 0 ? (uint32_t)nx_new : 0u;
    const uint32_t lm = (uint32_t)(len & 63);
    const uint32_t padlen = lm < 56 ? 56 - lm : 120 - lm;
    const uint32_t T = nxf + padlen + 8;
    if (T & 63) {
      status = EFES_ERR_STATE;
    } else {
      const uint64_t bits = len << 3;
      uint32_t hf[5] = {h[0], h[1], h[2], h[3], h[4]};
      for (uint32_t blk = 0; blk < T / 64; ++blk) {
        uint32_t w[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const uint32_t i = 64 * blk + 4 * k;
          w[k] = fin_byte(xl, i, nxf, T, bits) << 24 | fin_byte(xl, i + 1, nxf, T, bits) << 16 |
                 fin_byte(xl, i + 2, nxf, T, bits) << 8 | fin_byte(xl, i + 3, nxf, T, bits);
        }
        compress_inline(hf, w);
      }
#pragma unroll
      for (int k = 0; k < 5; ++k) dig[k] = hf[k];
    }
  }

  // ---- write back (a Sum-only job leaves the states alone: Go's Sum works on a copy)
  const bool keep = (jb.flags & EFES_JOB_SUM_ONLY) != 0;
  if (go) {
    if (do_sha && !keep) {
#pragma unroll
      for (int k = 0; k < 5; ++k) st->h[k] = h[k];
#pragma unroll
      for (int k = 0; k < 16; ++k)
        reinterpret_cast<uint32_t*>(st->x)[k] = (uint32_t)xl[4 * k] | (uint32_t)xl[4 * k + 1] << 8 |
                                                (uint32_t)xl[4 * k + 2] << 16 | (uint32_t)xl[4 * k + 3] << 24;
      st->nx = nx_new;
      st->len = len;
    }
    if (do_crc && !keep) cs->crc = ~crc_raw;
    if (fin && jb.sum) {
#pragma unroll
      for (int k = 0; k < 5; ++k) reinterpret_cast<uint32_t*>(jb.sum)[k] = bswap(status == EFES_OK ? dig[k] : 0u);
      reinterpret_cast<uint32_t*>(jb.sum)[5] = bswap(do_crc ? ~crc_raw : 0u);
    }
  }
  if (live && jb.status) *jb.status = bad ? EFES_ERR_STATE : status;
}


// ================================================================== synthetic fill
__device__ __forceinline__ uint64_t splitmix(uint64_t seed, uint64_t i) {
  uint64_t z = seed + (i + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void fill_kernel(uint64_t* __restrict__ dst, uint64_t nwords, uint64_t seed, uint8_t* tail_dst,
                            uint32_t tail_bytes) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += stride) dst[i] = splitmix(seed, i);
  if (blockIdx.x == 0 && threadIdx.x == 0 && tail_bytes) {
    const uint64_t z = splitmix(seed, nwords);
    for (uint32_t b = 0; b < tail_bytes; ++b) tail_dst[b] = (uint8_t)(z >> (8 * b));
  }
}

// ================================================================== launchers
hipError_t launch_deep(const efes_job* jobs, uint32_t njobs, const Tables* tabs, hipStream_t s) {
  if (njobs == 0) return hipSuccess;
  const uint32_t grid = (njobs + kPipeJobs - 1) / kPipeJobs;
  clear_last_error();
  hipLaunchKernelGGL(deep_kernel, dim3(grid), dim3(128 * kPipeJobs), 0, s, jobs, njobs, tabs);
  return hipGetLastError();
}


template <class K, class... A>
hipError_t launch_reserving(K kernel, dim3 grid, dim3 block, bool exclusive, hipStream_t s, const efes_job* jobs,
                            uint32_t njobs, const Tables* tabs, A... more) {
  size_t dyn = 0;
  if (exclusive) {
    hipFuncAttributes fa{};
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) == hipSuccess && fa.sharedSizeBytes < kCuLds) {
      dyn = kCuLds - fa.sharedSizeBytes;
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)dyn) != hipSuccess)
        dyn = 0;  // cannot reserve: run shared
    }
  }
  clear_last_error();
  hipLaunchKernelGGL(kernel, grid, block, dyn, s, jobs, njobs, tabs, more...);
  return hipGetLastError();
}

hipError_t launch_group(const efes_job* jobs, uint32_t njobs, int G, const Tables* tabs, hipStream_t s, bool exclusive) {
  if (njobs == 0) return hipSuccess;
  const uint32_t per_block = kDeepWaves * (64u / (uint32_t)G);
  const dim3 grid((njobs + per_block - 1) / per_block), block(64 * kDeepWaves);
  switch (G) {
    case 4: return launch_reserving(group_kernel<4>, grid, block, exclusive, s, jobs, njobs, tabs);
    case 8: return launch_reserving(group_kernel<8>, grid, block, exclusive, s, jobs, njobs, tabs);
    case 16: return launch_reserving(group_kernel<16>, grid, block, exclusive, s, jobs, njobs, tabs);
    case 32: return launch_reserving(group_kernel<32>, grid, block, exclusive, s, jobs, njobs, tabs);
    case 64: return launch_reserving(deep_kernel, dim3((njobs + kPipeJobs - 1) / kPipeJobs), dim3(128 * kPipeJobs),
                                     exclusive, s, jobs, njobs, tabs);
    default: return hipErrorInvalidValue;
  }
}

// FED shape of a mode: lanes per job and chain waves per workgroup.
constexpr int kFed4G = 4, kFed4C = 2;

template <int G, int C, bool X = false>
hipError_t launch_fed_shape(const efes_job* jobs, uint32_t njobs, const Tables* tabs, hipStream_t s) {
  const uint32_t per = C * (64 / G);
  return launch_reserving(fed_kernel<G, C, X>, dim3((njobs + per - 1) / per), dim3(256), true, s, jobs, njobs, tabs);
}

hipError_t launch_fed(const efes_job* jobs, uint32_t njobs, const Tables* tabs, hipStream_t s, bool expand) {
  if (njobs == 0) return hipSuccess;
  if (expand) return launch_fed_shape<4, 3, true>(jobs, njobs, tabs, s);  // FED4E
  return launch_fed_shape<kFed4G, kFed4C>(jobs, njobs, tabs, s);          // FED4
}

hipError_t launch_wide(const efes_job* jobs, uint32_t njobs, const Tables* tabs, hipStream_t s, bool exclusive,
                       int cus) {
  if (njobs == 0) return hipSuccess;
  // waves per SIMD of the launch: a workgroup per CU holds all of its SIMDs' waves (wide_pace);
  // exclusive parts (one wave per SIMD on reserved CUs) use 4-wave groups.
  const uint64_t waves = (njobs + 63) / 64, simds = 4ull * (uint64_t)(cus > 0 ? cus : 256);
  const uint32_t wps = exclusive ? 1u : (uint32_t)std::min<uint64_t>(kWideMaxWps, (waves + simds - 1) / simds);
  const uint32_t per = 64 * kWideWaves * wps;
  const size_t xs = (size_t)per * kXStride;  // the lanes' tail buffers (dynamic LDS)
  // The kernel's static LDS, and the dynamic-LDS limit raised once to the rest of the CU's LDS
  // (per launch `dyn` decides what a workgroup takes).
  // Per device (the attribute is set on the current one; the caller holds a DeviceGuard).
  static std::mutex mu;
  static int8_t ok_dev[64] = {};  // 0 = not tried, 1 = raised, -1 = failed
  static size_t static_lds = 0;
  int dev = 0;
  (void)hipGetDevice(&dev);
  bool big_ok = false;
  {
    std::lock_guard<std::mutex> lk(mu);
    int8_t& st = ok_dev[dev & 63];
    if (st == 0) {
      hipFuncAttributes fa{};
      st = -1;
      if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(wide_kernel)) == hipSuccess) {
        static_lds = fa.sharedSizeBytes;
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(wide_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kCuLds - static_lds)) == hipSuccess)
          st = 1;
      }
    }
    big_ok = st == 1;
  }
  // without the raised limit a workgroup gets 64 KiB of LDS in all (static: the CRC tables)
  if (!big_ok && sizeof(WideLDS) + xs > 64 * 1024) return hipErrorInvalidConfiguration;
  // exclusive: reserve the CU's whole LDS, so no other workgroup shares its SIMDs
  const size_t dyn = exclusive && big_ok ? kCuLds - static_lds : xs;
  clear_last_error();
  hipLaunchKernelGGL(wide_kernel, dim3((njobs + per - 1) / per), dim3(per), dyn, s, jobs, njobs, tabs);
  return hipGetLastError();
}

hipError_t launch_fill(void* dst, size_t bytes, uint64_t seed, hipStream_t s) {
  const uint64_t nwords = bytes / 8;
  const uint32_t tail = (uint32_t)(bytes % 8);
  uint64_t blocks = (nwords + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks == 0) blocks = 1;
  clear_last_error();
  hipLaunchKernelGGL(fill_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, reinterpret_cast<uint64_t*>(dst), nwords,
                     seed, reinterpret_cast<uint8_t*>(dst) + nwords * 8, tail);
  return hipGetLastError();
}

// ================================================================== chained jobs (efes_hash_chain)
// An object that lies in k extents is k Writes into one digest pair; through efes_hash_submit that is
// k stream-ordered launches, each as long as its longest job.  Here a job with EFES_JOB_CHAIN is the
// next Write into the states of the job before it, and one wavefront walks a whole chain: SHA-1 is
// serial within an object, not across objects.  Three stream-ordered launches over the caller's scratch:
//   * hash_chain_mark_kernel (one lane per job, 1024 jobs per workgroup): a job is a head when it is
//     job 0 or carries no EFES_JOB_CHAIN.  Writes the exclusive count of heads before each job within
//     its block (loc[]), the block's count (bsum[]), and zeroes the ticket.
//   * hash_chain_list_kernel (same grid): every workgroup sums the bsum[] of the blocks before it and
//     stores its heads' job indices at heads[base + loc], in job order; the last one stores the count.
//   * hash_chain_kernel (persistent; four waves per workgroup, one per SIMD, one workgroup per CU;
//     Tables in LDS once per workgroup, 64 B of x and 192 B of padding area per wave): a wave draws a chain with one atomic add
//     on the ticket (lane 0, broadcast), leaves when the ticket reaches the count, and runs the members
//     [heads[t], heads[t + 1]) in order through the one-wave job path, deep_head + deep_rest<true>,
//     exactly as a grouped wave runs a job that is left alone -- not deep_kernel's producer/consumer
//     pipeline, whose LDS hand-shake is per job.  An unflagged job is a chain of one and gets what
//     EFES_MODE_DEEP writes.  Validity is tracked on the way: a flagged job that is job 0, names other
//     states than the member before it, names none, carries INIT or SUM_ONLY, or follows a SUM_ONLY
//     job or an invalid member gets EFES_ERR_ARG and nothing else.
// The state stays in memory between members: deep_rest stores it with some lanes, the next deep_head
// loads it with all of them.  After each member the wave drains its stores, passes an agent-scope
// fence and waits again (the wait behind the fence is kept on purpose: the compiler may drop the
// fence's own).  The state pointers carry no const/__restrict__, so their loads stay vector loads,
// which the fence covers (scalar-cache loads it would not refresh).
// No wave waits for another: stream order is the only dependency between the launches and every loop
// bound comes from memory an earlier launch wrote, or from the ticket.  No LDS-DMA; the only inline
// assembly is that wait.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   hash_chain_mark_kernel    36 VGPRs,  16 SGPRs,     64 B LDS, no scratch, no spills, 8 waves/SIMD
//   hash_chain_list_kernel    18 VGPRs,  20 SGPRs,     64 B LDS, no scratch, no spills, 8 waves/SIMD
//   hash_chain_kernel        143 VGPRs, 106 SGPRs, 87 040 B LDS, no scratch, no VGPR spills, 2 SGPRs kept in
//                            VGPR lanes (as group_kernel<4>), 1 wave/SIMD (one workgroup per CU, by LDS)
// deep_kernel, group_kernel<*>, fed_kernel<*> and wide_kernel compile to the same registers, LDS, scratch
// and occupancy with and without this section.

// Sum of v over the workgroup's 1024 lanes, and this lane's exclusive prefix (wsum: 16 LDS words).
__device__ uint32_t chain_block_scan(uint32_t v, uint32_t* wsum, uint32_t* total) {
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
  for (uint32_t k = 0; k < kChainBlock / 64; ++k) {
    const uint32_t s = wsum[k];
    if (k < wave) base += s;
    tot += s;
  }
  __syncthreads();  // wsum may be written again
  *total = tot;
  return base + inc - v;
}

__device__ __forceinline__ bool chain_is_head(const efes_job* jobs, uint32_t j) {
  return j == 0u || (jobs[j].flags & EFES_JOB_CHAIN) == 0u;
}

__global__ __launch_bounds__(kChainBlock) void hash_chain_mark_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                                      void* scratch) {
  __shared__ uint32_t wsum[kChainBlock / 64];
  const HashChainScratch S = hash_chain_scratch_of(scratch, njobs);
  const uint32_t j = blockIdx.x * kChainBlock + threadIdx.x;
  const uint32_t head = j < njobs && chain_is_head(jobs, j) ? 1u : 0u;
  uint32_t total;
  const uint32_t excl = chain_block_scan(head, wsum, &total);
  if (j < njobs) S.loc[j] = excl;
  if (threadIdx.x == 0) {
    S.bsum[blockIdx.x] = total;
    if (blockIdx.x == 0) S.ctl->ticket = 0u;
  }
}

__global__ __launch_bounds__(kChainBlock) void hash_chain_list_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                                      void* scratch) {
  __shared__ uint32_t wsum[kChainBlock / 64];
  const HashChainScratch S = hash_chain_scratch_of(scratch, njobs);
  uint32_t base;  // heads in the blocks before this one
  (void)chain_block_scan(threadIdx.x < blockIdx.x ? S.bsum[threadIdx.x] : 0u, wsum, &base);
  const uint32_t j = blockIdx.x * kChainBlock + threadIdx.x;
  if (j < njobs && chain_is_head(jobs, j)) S.heads[base + S.loc[j]] = j;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) S.ctl->count = base + S.bsum[blockIdx.x];
}

struct ChainLDS {
  Tables tab;                    // 36 KiB
  uint8_t xs[kDeepWaves][64];    // each wave's tail buffer x
  uint8_t fin[kDeepWaves][192];  // padding assembly for checkSum
  // Never touched: lifts the workgroup over half of the CU's LDS, so a CU holds ONE of these workgroups
  // and a SIMD one chain.  By registers three would fit, and the tickets then put up to three chains on
  // one SIMD while others stay empty: 1024 chains of 4 MiB took 137 ms instead of 48, and 4096 chains
  // gained nothing (the SIMD's issue rate is the bound either way).  DESIGN.md §4 "Chained SHA-1 + CRC".
  uint8_t own_cu[48 * 1024];
};
static_assert(sizeof(ChainLDS) > kCuLds / 2 && sizeof(ChainLDS) <= 96 * 1024, "one chain workgroup per CU");

// The drain and agent-scope fence between a deep_rest and what loads the state it stored.
__device__ __forceinline__ void chain_fence() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One member's checkpoint (efes_hash_chain_checkpoints), behind a chain_fence() after the member's
// deep_rest<true>: the state deep_rest stored is read back, one 32-bit word per lane (the addresses differ
// by lane, so these are vector loads, which the fence covers), and all 28 words of the record are
// written -- zero for the _pad words and for the hash the chain does not keep.
__device__ __forceinline__ void chain_checkpoint(int lane, const DeepJob& J, efes_checkpoint* ck) {
  constexpr int kStateWords = (int)(sizeof(efes_sha1_state) / 4);
  constexpr int kPadWord = (int)(offsetof(efes_sha1_state, _pad) / 4);
  constexpr int kCrcWord = (int)(offsetof(efes_checkpoint, crc32) / 4);
  constexpr int kWords = (int)(sizeof(efes_checkpoint) / 4);
  static_assert(kCrcWord == kStateWords && kWords == kCrcWord + 2 && kWords <= 64, "one lane per word of the record");
  uint32_t* src = nullptr;
  if (lane < kStateWords && lane != kPadWord && J.st) src = reinterpret_cast<uint32_t*>(J.st) + lane;
  if (lane == kCrcWord && J.cs) src = &J.cs->crc;
  uint32_t v = 0u;
  if (src) v = *src;
  if (lane < kWords) reinterpret_cast<uint32_t*>(ck)[lane] = v;
}

// The wave walk.  kCkpt: also leave a checkpoint after every member that is due one (ckpt[j] != NULL, the
// Write took effect, no EFES_JOB_SUM_ONLY); without it ckpt is not read.
template <bool kCkpt>
__device__ __forceinline__ void hash_chain_walk(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                const Tables* __restrict__ tabs, void* scratch,
                                                efes_checkpoint* const* __restrict__ ckpt) {
  __shared__ __attribute__((aligned(16))) ChainLDS L;
  {
    const uint4* src = reinterpret_cast<const uint4*>(tabs);
    uint4* dst = reinterpret_cast<uint4*>(&L.tab);
    for (int i = threadIdx.x; i < (int)(sizeof(Tables) / 16); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int wave = (int)uniform32(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const HashChainScratch S = hash_chain_scratch_of(scratch, njobs);
  const uint32_t count = uniform32(S.ctl->count);
  for (;;) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(&S.ctl->ticket, 1u);
    t = uniform32(t);
    if (t >= count) break;
    const uint32_t first = uniform32(S.heads[t]);
    uint32_t end = njobs;
    if (t + 1u < count) end = uniform32(S.heads[t + 1u]);
    end = end < njobs ? end : njobs;
    bool bad = false, wrote = false;
    const efes_sha1_state* prev_st = nullptr;  // the member before: the states it names, its flags
    const efes_crc32_state* prev_cs = nullptr;
    uint32_t prev_flags = 0;
    for (uint32_t j = first; j < end; ++j) {
      const DeepJob J = load_job(jobs, j, lane);
      if (J.flags & EFES_JOB_CHAIN)  // j == first: job 0, a follower of nothing
        bad = bad || j == first || J.st != prev_st || J.cs != prev_cs || (J.st == nullptr && J.cs == nullptr) ||
              (J.flags & (EFES_JOB_INIT | EFES_JOB_SUM_ONLY)) != 0u || (prev_flags & EFES_JOB_SUM_ONLY) != 0u;
      if (bad) {  // not a Write into its chain's state: reported, nothing of it touched
        if (lane == 0 && J.status) *J.status = EFES_ERR_ARG;
        continue;
      }
      if (wrote) chain_fence();  // the member before stored the state this one loads
      const DeepMsg M = deep_head(L.tab, lane, J, L.xs[wave]);
      if (M.live) deep_rest<true>(L.tab, lane, J, L.xs[wave], L.fin[wave], M);
      wrote = true;
      if (kCkpt && M.live && (J.flags & EFES_JOB_SUM_ONLY) == 0u) {
        efes_checkpoint* ck = reinterpret_cast<efes_checkpoint*>(uniform64(reinterpret_cast<uint64_t>(ckpt[j])));
        if (ck) {
          chain_fence();
          chain_checkpoint(lane, J, ck);
          wrote = false;  // the fence has passed: the next member's stands here
        }
      }
      prev_st = J.st;
      prev_cs = J.cs;
      prev_flags = J.flags;
    }
  }
}

__global__ __launch_bounds__(64 * kDeepWaves) void hash_chain_kernel(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                                     const Tables* __restrict__ tabs, void* scratch) {
  hash_chain_walk<false>(jobs, njobs, tabs, scratch, nullptr);
}

size_t hash_chain_scratch_bytes(uint32_t njobs) {
  if (njobs == 0 || njobs > EFES_HASH_CHAIN_MAX_JOBS) return 0;
  const size_t b = sizeof(ChainCtl) + sizeof(uint32_t) * ((size_t)kChainMaxBlocks + 2 * (size_t)njobs);
  return (b + 15) & ~(size_t)15;
}

// The two prep launches: the chains' heads listed in the scratch, the ticket zeroed.
hipError_t launch_hash_chain_prep(const efes_job* jobs, uint32_t njobs, void* scratch, hipStream_t s) {
  const uint32_t nblocks = (njobs + kChainBlock - 1) / kChainBlock;
  clear_last_error();
  hipLaunchKernelGGL(hash_chain_mark_kernel, dim3(nblocks), dim3(kChainBlock), 0, s, jobs, njobs, scratch);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  clear_last_error();
  hipLaunchKernelGGL(hash_chain_list_kernel, dim3(nblocks), dim3(kChainBlock), 0, s, jobs, njobs, scratch);
  return hipGetLastError();
}

hipError_t launch_hash_chain(const efes_job* jobs, uint32_t njobs, void* scratch, const Tables* tabs, int cus,
                             hipStream_t s) {
  if (njobs == 0) return hipSuccess;
  const hipError_t e = launch_hash_chain_prep(jobs, njobs, scratch, s);
  if (e != hipSuccess) return e;
  // Persistent grid: the chain count lives on the device, so the grid is sized by the job count and
  // by what is resident at once (a workgroup that starts late finds the tickets gone and leaves).
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, hash_chain_kernel, 64 * kDeepWaves, 0) != hipSuccess ||
      per_cu < 1)
    per_cu = 1;
  const uint64_t resident = (uint64_t)(cus > 0 ? cus : 256) * (uint64_t)per_cu;
  const uint64_t want = ((uint64_t)njobs + kDeepWaves - 1) / kDeepWaves;
  clear_last_error();
  hipLaunchKernelGGL(hash_chain_kernel, dim3((uint32_t)std::min(want, resident)), dim3(64 * kDeepWaves), 0, s, jobs,
                     njobs, tabs, scratch);
  return hipGetLastError();
}

// ------------------------------------------------------------------ grouped walk (efes_hash_chain_mode)
// For more chains than SIMDs: the same prep launches, scratch, ticket and heads[] list, then a persistent
// launch of group_kernel's workgroup (four waves, one per SIMD; Tables + PosTables, msg, xs and fin in
// LDS, over half a CU's LDS, so a workgroup owns its CU).  A wave has 64/G slots and each slot holds one
// chain: its ticket range [cur, end), the validity state the wave walk keeps, and the DeepMsg of its
// current member.  The wave alternates two steps, all of it wave-uniform:
//   1. refill: every slot without a joinable member (>= G bulk blocks left) is driven on -- a headed
//      member with fewer than G blocks left is finished by deep_rest<true>, the cursor advances, at a
//      chain's end the slot draws the next chain (one atomic add by lane 0, broadcast; the wave's first
//      64/G tickets come from one add; a spent ticket leaves the slot dead: DeepMsg{}), each new member
//      is checked by the wave walk's rules (invalid: EFES_ERR_ARG and nothing else) and gets deep_head
//      into the slot's xs.  The wave walk's drain and agent-scope fence stand before every deep_head
//      that follows a deep_rest of this wave.
//   2. joint round: with no joiner the wave leaves; a lone joiner (every other slot is then dead) goes
//      back through step 1, which finishes it on the one-job path; two or more advance together by S*G
//      blocks through group_bulk_any, S the smallest left/G among them, then step 1 again.
// No wave waits for another; every loop bound comes from memory an earlier launch wrote, or from the
// ticket.  No LDS-DMA; the only inline assembly is the wave walk's wait.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   hash_chain_group_kernel<4>    215 VGPRs, 106 SGPRs, 114 432 B LDS, no scratch, no VGPR spills, 52 SGPRs kept in VGPR lanes
//   hash_chain_group_kernel<8>    215 VGPRs, 106 SGPRs, 114 432 B LDS, no scratch, no VGPR spills, 49 SGPRs kept in VGPR lanes
//   hash_chain_group_kernel<16>   215 VGPRs, 106 SGPRs, 114 432 B LDS, no scratch, no VGPR spills, 51 SGPRs kept in VGPR lanes
//   hash_chain_group_kernel<32>   217 VGPRs, 106 SGPRs, 114 432 B LDS, no scratch, no VGPR spills, 53 SGPRs kept in VGPR lanes
//   each 1 wave/SIMD (one workgroup per CU, by LDS), no AGPRs.
// deep_kernel, group_kernel<*>, fed_kernel<*>, wide_kernel and hash_chain_kernel compile to the same
// registers, LDS, scratch and occupancy with and without this section.  That needs group_bulk's kUser: with
// a second caller of one instantiation the compiler stops inlining it into group_kernel as well (248 VGPRs
// + 32 AGPRs, 180-260 B of scratch per lane in both kernels).
struct ChainSlot {
  uint32_t cur, end;    // the chain's members not yet finished: jobs [cur, end)
  uint32_t first;       // the chain's head
  uint32_t bad;         // an invalid member was met: the members behind it are invalid too
  uint32_t prev_flags;  // the valid member before: its flags and the states it names
  uint32_t pad;
  const efes_sha1_state* prev_st;
  const efes_crc32_state* prev_cs;
};
struct ChainGroupLDS {
  DeepLDS d;
  ChainSlot slot[kDeepWaves][kGroupMaxJobs];
};
static_assert(sizeof(ChainGroupLDS) > kCuLds / 2 && sizeof(ChainGroupLDS) <= kCuLds, "one workgroup per CU");

template <int G, bool kCkpt>
__device__ __forceinline__ void hash_chain_group_walk(const efes_job* __restrict__ jobs, uint32_t njobs,
                                                      const Tables* __restrict__ tabs, void* scratch,
                                                      efes_checkpoint* const* __restrict__ ckpt) {
  constexpr int kSlots = 64 / G;
  static_assert(kSlots <= kGroupMaxJobs, "LDS holds kGroupMaxJobs slots per wave");
  __shared__ __attribute__((aligned(16))) ChainGroupLDS L;
  {
    const uint4* src = reinterpret_cast<const uint4*>(tabs);  // Tables then PosTables
    uint4* dst = reinterpret_cast<uint4*>(&L.d.tab);
    for (int i = threadIdx.x; i < (int)((sizeof(Tables) + sizeof(PosTables)) / 16); i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  const int wave = (int)uniform32(threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const HashChainScratch S = hash_chain_scratch_of(scratch, njobs);
  const uint32_t count = uniform32(S.ctl->count);
  DeepMsg* msgs = L.d.msg[wave];
  ChainSlot* slots = L.slot[wave];
  if (lane < kSlots) {
    msgs[lane] = DeepMsg{};
    slots[lane] = ChainSlot{};
  }
  wave_lds_sync();
  // A wave's first draw is one atomic add for all its slots, so that it starts with consecutive chains
  // (of similar lengths in an array sorted longest first, as the grouped job kernels expect) and two
  // chains of a small array meet in one wave; every later draw is one ticket for one slot.
  uint32_t pre = 0;
  if (lane == 0) pre = atomicAdd(&S.ctl->ticket, (uint32_t)kSlots);
  pre = uniform32(pre);
  const uint32_t pre_end = pre + (uint32_t)kSlots;
  bool spent = false;  // the ticket has reached the count: no slot of this wave draws again
  bool wrote = false;  // a deep_rest of this wave stored a state since the last fence
  int lone = -1;       // the slot whose member was left alone by the last step 2
  for (;;) {
    // ---- step 1: refill
    for (int m = 0; m < kSlots; ++m) {
      const bool live0 = uniform32(msgs[m].live) != 0u;
      if (live0 && m != lone && uniform64(msgs[m].nbulk) - uniform64(msgs[m].done) >= (uint64_t)G) continue;
      ChainSlot C;
      C.cur = uniform32(slots[m].cur);
      C.end = uniform32(slots[m].end);
      if (!live0 && spent && C.cur >= C.end) continue;  // dead
      C.first = uniform32(slots[m].first);
      C.bad = uniform32(slots[m].bad);
      C.prev_flags = uniform32(slots[m].prev_flags);
      C.pad = 0;
      C.prev_st = reinterpret_cast<const efes_sha1_state*>(uniform64(reinterpret_cast<uint64_t>(slots[m].prev_st)));
      C.prev_cs = reinterpret_cast<const efes_crc32_state*>(uniform64(reinterpret_cast<uint64_t>(slots[m].prev_cs)));
      DeepMsg M = uniform_msg(msgs[m]);
      for (;;) {
        if (M.live) {
          if (m != lone && M.nbulk - M.done >= (uint64_t)G) break;  // joinable
          const DeepJob Jr = load_job(jobs, C.cur, lane);
          deep_rest<true>(L.d.tab, lane, Jr, L.d.xs[wave][m], L.d.fin[wave], M);
          wrote = true;
          if (kCkpt && (Jr.flags & EFES_JOB_SUM_ONLY) == 0u) {
            efes_checkpoint* ck =
                reinterpret_cast<efes_checkpoint*>(uniform64(reinterpret_cast<uint64_t>(ckpt[C.cur])));
            if (ck) {
              chain_fence();
              chain_checkpoint(lane, Jr, ck);
              wrote = false;
            }
          }
          M = DeepMsg{};
          ++C.cur;
        }
        if (C.cur >= C.end) {  // the chain's end: the next chain
          uint32_t t = 0;
          if (!spent) {
            if (pre < pre_end) {
              t = pre++;
            } else {
              if (lane == 0) t = atomicAdd(&S.ctl->ticket, 1u);
              t = uniform32(t);
            }
            spent = t >= count;
          }
          if (spent) break;  // dead: M is DeepMsg{}
          C.first = uniform32(S.heads[t]);
          uint32_t end = njobs;
          if (t + 1u < count) end = uniform32(S.heads[t + 1u]);
          C.end = end < njobs ? end : njobs;
          C.cur = C.first;
          C.bad = 0u;
          C.prev_flags = 0u;
          C.prev_st = nullptr;
          C.prev_cs = nullptr;
          if (C.cur >= C.end) continue;
        }
        const DeepJob J = load_job(jobs, C.cur, lane);
        if (J.flags & EFES_JOB_CHAIN)  // cur == first: job 0, a follower of nothing
          C.bad |= (C.cur == C.first || J.st != C.prev_st || J.cs != C.prev_cs || (J.st == nullptr && J.cs == nullptr) ||
                    (J.flags & (EFES_JOB_INIT | EFES_JOB_SUM_ONLY)) != 0u || (C.prev_flags & EFES_JOB_SUM_ONLY) != 0u)
                       ? 1u
                       : 0u;
        if (C.bad) {  // not a Write into its chain's state: reported, nothing of it touched
          if (lane == 0 && J.status) *J.status = EFES_ERR_ARG;
          ++C.cur;
          continue;
        }
        if (wrote) {  // a member before stored the state this one may load
          chain_fence();
          wrote = false;
        }
        M = deep_head(L.d.tab, lane, J, L.d.xs[wave][m]);
        C.prev_st = J.st;
        C.prev_cs = J.cs;
        C.prev_flags = J.flags;
        if (!M.live) ++C.cur;  // Go panicked at the Write: the status is written, nothing else
      }
      wave_lds_sync();
      if (lane == 0) {
        msgs[m] = M;
        slots[m] = C;
      }
    }
    lone = -1;
    wave_lds_sync();

    // ---- step 2: joint round of the slots whose member has >= G bulk blocks left
    uint64_t St = ~0ull;
    int joiners = 0;
    bool any_sha = false, any_crc = false, all16 = true;
    for (int m = 0; m < kSlots; ++m) {
      const uint64_t left = uniform32(msgs[m].live) ? (uniform64(msgs[m].nbulk) - uniform64(msgs[m].done)) / G : 0;
      if (lane == 0) msgs[m].joint = left ? 1u : 0u;
      if (left == 0) continue;
      ++joiners;
      lone = m;
      St = left < St ? left : St;
      const DeepJob J = load_job(jobs, uniform32(slots[m].cur), lane);
      any_sha |= J.st != nullptr;
      any_crc |= J.cs != nullptr;
      const uint8_t* q = reinterpret_cast<const uint8_t*>(uniform64(reinterpret_cast<uint64_t>(msgs[m].q)));
      all16 &= (reinterpret_cast<uintptr_t>(q + 64 * uniform64(msgs[m].done)) & 15) == 0;
    }
    if (joiners == 0) break;
    if (joiners == 1) continue;  // step 1 runs slot `lone` to its member's end on the one-job path
    lone = -1;
    wave_lds_sync();
    constexpr int kUser = kCkpt ? 2 : 1;  // an instantiation of group_bulk for each kernel (see Resources above)
    if (all16) group_bulk_any<G, true, kUser>(L.d.tab, L.d.pos, lane, msgs, St, any_sha, any_crc);
    else group_bulk_any<G, false, kUser>(L.d.tab, L.d.pos, lane, msgs, St, any_sha, any_crc);
  }
}

template <int G>
__global__ __launch_bounds__(64 * kDeepWaves, 1) void hash_chain_group_kernel(const efes_job* __restrict__ jobs,
                                                                              uint32_t njobs,
                                                                              const Tables* __restrict__ tabs,
                                                                              void* scratch) {
  hash_chain_group_walk<G, false>(jobs, njobs, tabs, scratch, nullptr);
}

template <int G>
hipError_t launch_hash_chain_group_shape(const efes_job* jobs, uint32_t njobs, void* scratch, const Tables* tabs,
                                         int cus, hipStream_t s) {
  // Persistent grid, as the wave walk's: the workgroups that njobs chains would fill, or what is resident.
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, hash_chain_group_kernel<G>, 64 * kDeepWaves, 0) !=
          hipSuccess ||
      per_cu < 1)
    per_cu = 1;
  const uint64_t resident = (uint64_t)(cus > 0 ? cus : 256) * (uint64_t)per_cu;
  const uint64_t per_block = (uint64_t)kDeepWaves * (64 / G);
  const uint64_t want = ((uint64_t)njobs + per_block - 1) / per_block;
  clear_last_error();
  hipLaunchKernelGGL(hash_chain_group_kernel<G>, dim3((uint32_t)std::min(want, resident)), dim3(64 * kDeepWaves), 0, s,
                     jobs, njobs, tabs, scratch);
  return hipGetLastError();
}

hipError_t launch_hash_chain_group(const efes_job* jobs, uint32_t njobs, int G, void* scratch, const Tables* tabs,
                                   int cus, hipStream_t s) {
  if (njobs == 0) return hipSuccess;
  if (G != 4 && G != 8 && G != 16 && G != 32) return hipErrorInvalidValue;
  const hipError_t e = launch_hash_chain_prep(jobs, njobs, scratch, s);
  if (e != hipSuccess) return e;
  switch (G) {
    case 4: return launch_hash_chain_group_shape<4>(jobs, njobs, scratch, tabs, cus, s);
    case 8: return launch_hash_chain_group_shape<8>(jobs, njobs, scratch, tabs, cus, s);
    case 16: return launch_hash_chain_group_shape<16>(jobs, njobs, scratch, tabs, cus, s);
    default: return launch_hash_chain_group_shape<32>(jobs, njobs, scratch, tabs, cus, s);
  }
}

// ------------------------------------------------------------------ checkpoints (efes_hash_chain_checkpoints)
// The resumable state after every member the caller asks for: the same prep launches, scratch, ticket and
// heads[] list, then the wave walk or the grouped walk instantiated with kCkpt -- kernels of their own, so
// hash_chain_kernel and hash_chain_group_kernel<*> stay the code they were.  Where a member ends in
// deep_rest<true> (the wave walk's loop; step 1 of the grouped walk) and is due a record, the wave passes
// the walks' drain and agent-scope fence at once instead of before the next deep_head, reads the stored
// state back (chain_checkpoint: one word per lane, vector loads through the non-const state pointers) and
// stores the 28 words of the record.  deep_rest itself is untouched: it is shared with the job kernels,
// and the record needs nothing it does not already store.  The fence is the one the next member of this
// wave would have passed anyway, so a checkpoint costs one load and one store round trip per member and
// one more fence per chain (after its last member).  A member that is invalid, whose Write panics in Go
// (deep_head's live == 0) or that carries EFES_JOB_SUM_ONLY never reaches the store; ckpt[] is read only
// for members that do.  No wave waits for another; every loop bound comes from memory an earlier launch
// wrote, or from the ticket; no LDS-DMA; the only inline assembly is the walks' wait.
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   hash_chain_ckpt_kernel            144 VGPRs, 106 SGPRs,  87 040 B LDS, no scratch, no VGPR spills, 14 SGPRs kept in VGPR lanes
//   hash_chain_group_ckpt_kernel<4>   215 VGPRs, 106 SGPRs, 114 432 B LDS, no scratch, no VGPR spills, 59 SGPRs kept in VGPR lanes
//   hash_chain_group_ckpt_kernel<8>   217 VGPRs, 106 SGPRs, 114 432 B LDS, no scratch, no VGPR spills, 59 SGPRs kept in VGPR lanes
//   hash_chain_group_ckpt_kernel<16>  217 VGPRs, 106 SGPRs, 114 432 B LDS, no scratch, no VGPR spills, 65 SGPRs kept in VGPR lanes
//   hash_chain_group_ckpt_kernel<32>  217 VGPRs, 106 SGPRs, 114 432 B LDS, no scratch, no VGPR spills, 61 SGPRs kept in VGPR lanes
//   the five walks each 1 wave/SIMD (one workgroup per CU, by LDS), no AGPRs.
//   checkpoint_text_kernel              8 VGPRs,  18 SGPRs,       0 B LDS, no scratch, no spills, 8 waves/SIMD
// Every other kernel of this file compiles to the same registers, LDS, scratch and occupancy with and
// without this section (group_bulk's kUser = 2 keeps the grouped walks' bulk step apart).
__global__ __launch_bounds__(64 * kDeepWaves) void hash_chain_ckpt_kernel(const efes_job* __restrict__ jobs,
                                                                          uint32_t njobs,
                                                                          const Tables* __restrict__ tabs,
                                                                          void* scratch,
                                                                          efes_checkpoint* const* __restrict__ ckpt) {
  hash_chain_walk<true>(jobs, njobs, tabs, scratch, ckpt);
}

template <int G>
__global__ __launch_bounds__(64 * kDeepWaves, 1) void hash_chain_group_ckpt_kernel(
    const efes_job* __restrict__ jobs, uint32_t njobs, const Tables* __restrict__ tabs, void* scratch,
    efes_checkpoint* const* __restrict__ ckpt) {
  hash_chain_group_walk<G, true>(jobs, njobs, tabs, scratch, ckpt);
}

// The persistent grid of a walk: the workgroups that njobs chains would fill, or what is resident.
template <typename Kernel>
static uint32_t chain_ckpt_grid(Kernel kernel, uint32_t njobs, uint64_t per_block, int cus) {
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64 * kDeepWaves, 0) != hipSuccess || per_cu < 1)
    per_cu = 1;
  const uint64_t resident = (uint64_t)(cus > 0 ? cus : 256) * (uint64_t)per_cu;
  const uint64_t want = ((uint64_t)njobs + per_block - 1) / per_block;
  return (uint32_t)std::min(want, resident);
}

template <int G>
static hipError_t launch_hash_chain_group_ckpt_shape(const efes_job* jobs, uint32_t njobs, void* scratch,
                                                     const Tables* tabs, int cus, efes_checkpoint* const* ckpt,
                                                     hipStream_t s) {
  const uint32_t grid = chain_ckpt_grid(hash_chain_group_ckpt_kernel<G>, njobs, (uint64_t)kDeepWaves * (64 / G), cus);
  clear_last_error();
  hipLaunchKernelGGL(hash_chain_group_ckpt_kernel<G>, dim3(grid), dim3(64 * kDeepWaves), 0, s, jobs, njobs, tabs,
                     scratch, ckpt);
  return hipGetLastError();
}

hipError_t launch_hash_chain_ckpt(const efes_job* jobs, uint32_t njobs, int G, efes_checkpoint* const* ckpt,
                                  void* scratch, const Tables* tabs, int cus, hipStream_t s) {
  if (njobs == 0) return hipSuccess;
  if (G != 0 && G != 4 && G != 8 && G != 16 && G != 32) return hipErrorInvalidValue;
  const hipError_t e = launch_hash_chain_prep(jobs, njobs, scratch, s);
  if (e != hipSuccess) return e;
  switch (G) {
    case 0: {
      const uint32_t grid = chain_ckpt_grid(hash_chain_ckpt_kernel, njobs, kDeepWaves, cus);
      clear_last_error();
      hipLaunchKernelGGL(hash_chain_ckpt_kernel, dim3(grid), dim3(64 * kDeepWaves), 0, s, jobs, njobs, tabs, scratch,
                         ckpt);
      return hipGetLastError();
    }
    case 4: return launch_hash_chain_group_ckpt_shape<4>(jobs, njobs, scratch, tabs, cus, ckpt, s);
    case 8: return launch_hash_chain_group_ckpt_shape<8>(jobs, njobs, scratch, tabs, cus, ckpt, s);
    case 16: return launch_hash_chain_group_ckpt_shape<16>(jobs, njobs, scratch, tabs, cus, ckpt, s);
    default: return launch_hash_chain_group_ckpt_shape<32>(jobs, njobs, scratch, tabs, cus, ckpt, s);
  }
}

// The `.info` text of n records (efes_checkpoints_marshal_text): one lane per byte of the 104 that
// MarshalText encodes -- h big-endian, x as it lies, nx and len big-endian (sha1_efes.go:26-34), then the
// CRC big-endian (crc32_efes.go:18-24) -- which it reads from the record and writes as two lower-case hex
// characters.  efes_sha1_state_marshal_text / efes_crc32_state_marshal_text (efes_api.cpp) are the
// specification.
constexpr uint32_t kCkptTextBlock = 256;
constexpr uint32_t kCkptBinBytes = EFES_CHECKPOINT_TEXT_BYTES / 2;  // 100 of the SHA-1 state + 4 of the CRC
static_assert(kCkptBinBytes == 104 && (uint64_t)EFES_HASH_CHAIN_MAX_JOBS * kCkptBinBytes < (1ull << 32),
              "checkpoint_text_kernel indexes the bytes with 32 bits");

__global__ __launch_bounds__(kCkptTextBlock) void checkpoint_text_kernel(const efes_checkpoint* __restrict__ ckpt,
                                                                         uint32_t n, char* __restrict__ text) {
  const uint32_t t = blockIdx.x * kCkptTextBlock + threadIdx.x;
  if (t >= n * kCkptBinBytes) return;
  const uint32_t i = t / kCkptBinBytes, k = t - i * kCkptBinBytes;
  uint32_t at;  // the byte of the record that MarshalText puts at position k
  if (k < 20u) at = (k & ~3u) + (3u - (k & 3u));                                        // h[k / 4]
  else if (k < 84u) at = (uint32_t)offsetof(efes_sha1_state, x) + (k - 20u);            // x
  else if (k < 92u) at = (uint32_t)offsetof(efes_sha1_state, nx) + (7u - (k - 84u));    // nx
  else if (k < 100u) at = (uint32_t)offsetof(efes_sha1_state, len) + (7u - (k - 92u));  // len
  else at = (uint32_t)offsetof(efes_checkpoint, crc32) + (3u - (k - 100u));             // crc
  const uint32_t b = reinterpret_cast<const uint8_t*>(ckpt + i)[at];
  const uint32_t hi = b >> 4, lo = b & 15u;
  char* out = text + (size_t)i * EFES_CHECKPOINT_TEXT_BYTES + 2u * k;
  out[0] = (char)(hi < 10u ? '0' + hi : 'a' + (hi - 10u));
  out[1] = (char)(lo < 10u ? '0' + lo : 'a' + (lo - 10u));
}

hipError_t launch_checkpoint_text(const efes_checkpoint* ckpt, uint32_t n, char* text, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t total = n * kCkptBinBytes;
  clear_last_error();
  hipLaunchKernelGGL(checkpoint_text_kernel, dim3((total + kCkptTextBlock - 1) / kCkptTextBlock), dim3(kCkptTextBlock),
                     0, s, ckpt, n, text);
  return hipGetLastError();
}

}  // namespace efes
