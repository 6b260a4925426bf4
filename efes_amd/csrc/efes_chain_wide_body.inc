// efes_chain_wide_body.inc -- the body of the wide chain walk, included into the kernels that run it:
// hash_chain_wide_kernel<kCkpt> (efes_chain_wide.hip, kCopy false) and hash_chain_wide_copy_kernel<kCkpt>
// (efes_chain_wide_copy.hip, kCopy true).  It is text, not a function: as an inlined function the same
// statements gave hash_chain_wide_kernel 148 VGPRs and another instruction stream, and that kernel keeps the
// code it was measured with (147 VGPRs, profiles/hash_chain_wide/resources.txt).  The including kernel
// provides: jobs, njobs, tabs, scratch, ckpt, dsts (NULL without kCopy), the constants kCkpt and kCopy, the
// static LDS `L` (WideLDS) and the dynamic LDS `chain_wide_xs` (blockDim.x x kXStride bytes).
//
// ------------------------------------------------------------------ wide walk (efes_hash_chain_wide, efes_hash_chain_wide_copy)
// For very many chains of short members: the same prep launches, scratch, ticket and heads[] list, then a
// persistent launch of wide_kernel's workgroup (4 x wps waves, one workgroup per CU; the position tables
// in static LDS, a 68-byte-stride tail buffer per lane in dynamic LDS).  A wave draws 64 consecutive
// chains with one atomic add of 64 on the ticket (lane 0, broadcast); lane l owns chain t + l while that is below
// the count, members [heads[c], heads[c + 1]), the last chain ending at njobs.  The wave then walks in
// rounds: round r is every lane's r-th member, and the wave loops to its longest chain.  The host sizes the
// workgroup from njobs, the only bound it has; the kernel knows the chain count, and the waves per SIMD that
// the chains cannot fill leave behind the table load's barrier, before any draw (with them, 65 536 chains of
// 4 members -- 1024 waves of chains in a launch of 3072 -- took 4.0 ms instead of 1.6: the workgroups that
// started first drew three waves of chains per SIMD and other CUs none).  Round 0 loads the
// state (or takes NewSha1's); every round is what wide_kernel does for a job -- byte-wise head into x,
// wide_bulk_any over the round's per-lane block counts with its uniform and ragged phases, tail, Sum on a
// copy, sum and status -- with the wave walk's validity rules kept per lane.  h, nx, len and the raw CRC
// stay in registers and x in the lane's LDS buffer between members, which makes the stale bytes x[nx:64]
// those of successive Writes; the state is stored once, behind the chain's last member, when a Write that
// is not EFES_JOB_SUM_ONLY took effect.  Nothing of a chain is read back from memory, so no fence stands
// between members.  kCkpt: after every member that is due a record (the Write took effect, no
// EFES_JOB_SUM_ONLY, ckpt[j] != NULL; ckpt[] is read for no other member) the lane stores the 28 words of
// the record from its registers and LDS, zero for the _pad words and for a hash the chain does not keep.
// kCopy: a member whose Write takes effect (`go`) and is not EFES_JOB_SUM_ONLY, on a chain that names a state,
// with dsts[j] != NULL, is also stored at dsts[j], byte for byte, from the registers it is hashed from: the head bytes beside the
// loads that complete x, whole blocks in wide_bulk_copy, the tail bytes one by one.  The lane knows `go`
// before it touches the member, so nothing is written for an invalid member, for one whose Write panics or
// for the members behind it.  Without kCopy nothing of dsts is left in the kernel.
// No wave waits for another: the only barrier stands behind the table load, before any draw; wide_pace
// only sets priorities; every loop bound comes from the ticket, from count and heads[] that an earlier
// launch wrote, or from the job records.  No LDS-DMA, no inline assembly beyond wide_step's register pin.
// A wave lasts as long as the sum over rounds of its longest member: arrays sorted longest first keep
// that small, as for wide_kernel.
  {
    const uint4* src = wide_tab_src(tabs);
    uint4* dst = reinterpret_cast<uint4*>(L.crc);
    for (int i = threadIdx.x; i < (int)(sizeof(L.crc) / 16); i += blockDim.x) dst[i] = src[i];
    if (threadIdx.x < kWideWaves * kWideMaxWps) L.prog[threadIdx.x] = 0;
  }
  __syncthreads();
  const uint32_t wv = threadIdx.x / 64;
  const uint32_t lane = threadIdx.x & 63u;
  uint8_t* xl = chain_wide_xs + (size_t)threadIdx.x * kXStride;
  const HashChainScratch S = hash_chain_scratch_of(scratch, njobs);
  const uint32_t count = uniform32(S.ctl->count);
  // The host sized the workgroup by njobs; the chain count is known here.  The waves per SIMD that the
  // chains can fill stay, the others leave before any draw (the barrier is behind them): otherwise the
  // first workgroups to start would take three waves of chains per SIMD and leave other CUs without any.
  const uint32_t simds = kWideWaves * gridDim.x, need = (count + 63u) / 64u;
  uint32_t wps = (need + simds - 1u) / simds;
  wps = wps < 1u ? 1u : wps;
  const uint32_t nwv = blockDim.x / 64 < kWideWaves * wps ? blockDim.x / 64 : kWideWaves * wps;
  if (wv >= nwv) return;
  const uint8_t* dummy = reinterpret_cast<const uint8_t*>(tabs);  // 36 KiB of valid device memory
  for (;;) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(&S.ctl->ticket, 64u);
    t = uniform32(t);
    if (t >= count) break;
    const uint32_t c = t + lane;
    uint32_t cur = 0, end = 0;  // this lane's members not yet run: jobs [cur, end)
    if (c < count) {
      cur = S.heads[c];
      end = c + 1u < count ? S.heads[c + 1u] : njobs;
      end = end < njobs ? end : njobs;
    }
    // the chain's state (registers; x in xl) and what the wave walk keeps of the members before
    uint32_t h[5] = {0, 0, 0, 0, 0};
    int64_t nx = 0;
    uint64_t len = 0;
    uint32_t crc_raw = 0;
    efes_sha1_state* st = nullptr;  // the states the head names: every valid member names the same
    efes_crc32_state* cs = nullptr;
    uint32_t prev_flags = 0;
    bool bad = false;    // an invalid member was met: the members behind it are invalid too
    bool dirty = false;  // a Write other than EFES_JOB_SUM_ONLY took effect: the state is stored at the end
    for (bool head = true; __any(cur < end); head = false) {
      const bool active = cur < end;
      const efes_job jb = active ? jobs[cur] : efes_job{};
      const uint32_t flags = jb.flags;
      if (head) {
        st = jb.sha1;
        cs = jb.crc32;
      }
      if (active && (flags & EFES_JOB_CHAIN))  // head: job 0, a follower of nothing
        bad = bad || head || jb.sha1 != st || jb.crc32 != cs || (jb.sha1 == nullptr && jb.crc32 == nullptr) ||
              (flags & (EFES_JOB_INIT | EFES_JOB_SUM_ONLY)) != 0u || (prev_flags & EFES_JOB_SUM_ONLY) != 0u;
      if (active && bad && jb.status) *jb.status = EFES_ERR_ARG;  // reported, nothing else of it touched
      const bool valid = active && !bad;
      const bool do_sha = valid && st != nullptr, do_crc = valid && cs != nullptr;
      const bool fin = valid && (flags & EFES_JOB_FINALIZE) != 0;
      const bool keep = (flags & EFES_JOB_SUM_ONLY) != 0;
      if (valid) prev_flags = flags;
      const uint8_t* p = reinterpret_cast<const uint8_t*>(jb.data);
      const uint64_t plen = jb.length;
      int32_t status = EFES_OK;

      if (head) {  // wave-uniform: round 0 is every lane's head
        const bool init = valid && (flags & EFES_JOB_INIT) != 0;
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
        crc_raw = do_crc ? (init ? 0xFFFFFFFFu : ~cs->crc) : 0u;
      }
      const bool go = valid && !(do_sha && nx > 64);  // sha1.go:62 panic: this member and its followers

      // kCopy: where this member's bytes go, NULL when it is not copied: its Write does not take effect, the chain
      // names no state, or it is an EFES_JOB_SUM_ONLY job, whose Write is to a copy of the digests (length 0 by
      // its definition).  dsts[] is read for no other member.
      uint8_t* dp = nullptr;
      if constexpr (kCopy) {
        if (go && !keep && (do_sha || do_crc)) dp = static_cast<uint8_t*>(dsts[cur]);
      }

      // ---- head
      uint64_t pos = 0;
      if (go && do_sha && nx > 0) {
        const uint32_t room = (uint32_t)(64 - nx);
        const uint32_t nh = plen < room ? (uint32_t)plen : room;
        if constexpr (kCopy) {
          for (uint32_t i = 0; i < nh; ++i) {
            const uint32_t v = ldg_u8(p + i);
            xl[nx + i] = (uint8_t)v;
            if (dp) stg_u8(dp + i, v);
          }
        } else {
          for (uint32_t i = 0; i < nh; ++i) xl[nx + i] = ldg_u8(p + i);
        }
        if ((uint32_t)nx + nh == 64) {
          uint32_t w[16];
#pragma unroll
          for (int k = 0; k < 16; ++k) w[k] = be_word_lds(xl, k);
          compress_inline(h, w);
          nx = 0;
        } else {
          nx += nh;
        }
        pos = nh;
      }
      if (go && do_crc)
        for (uint64_t i = 0; i < pos; ++i) crc_raw = crc_byte(wide_t0(L), crc_raw, ldg_u8(p + i));

      // ---- bulk: the round's per-lane block counts (masked when done)
      const uint8_t* q = p + pos;
      const uint64_t nbulk = go ? (plen - pos) >> 6 : 0;
      const bool all16 = __all(!go || (reinterpret_cast<uintptr_t>(q) & 15) == 0);
      const bool any_sha = __any(go && do_sha), any_crc = __any(go && do_crc);  // wave-uniform
      const uint64_t nmax = wave_max64(nbulk);
      // the shortest member over ALL lanes (a lane without one has nbulk 0: no uniform phase)
      const uint64_t nmin = wave_min64(nbulk, true);
      if constexpr (kCopy) {
        // an address, not dp + pos: dp may be NULL, and then nothing is stored through dq
        uint8_t* dq = reinterpret_cast<uint8_t*>(reinterpret_cast<uintptr_t>(dp) + pos);
        if (all16) wide_bulk_copy_any<true>(q, dq, dp != nullptr, nbulk, nmin, nmax, dummy, any_sha, any_crc, L.crc, h, crc_raw, L.prog, wv, nwv);
        else wide_bulk_copy_any<false>(q, dq, dp != nullptr, nbulk, nmin, nmax, dummy, any_sha, any_crc, L.crc, h, crc_raw, L.prog, wv, nwv);
      } else {
        if (all16) wide_bulk_any<true>(q, nbulk, nmin, nmax, dummy, any_sha, any_crc, L.crc, h, crc_raw, L.prog, wv, nwv);
        else wide_bulk_any<false>(q, nbulk, nmin, nmax, dummy, any_sha, any_crc, L.crc, h, crc_raw, L.prog, wv, nwv);
      }

      // ---- tail
      const uint64_t tpos = pos + (nbulk << 6);
      const uint32_t r = go ? (uint32_t)(plen - tpos) : 0u;
      if (do_crc)
        for (uint32_t i = 0; i < r; ++i) crc_raw = crc_byte(wide_t0(L), crc_raw, ldg_u8(p + tpos + i));
      if (do_sha && r > 0) {
        for (uint32_t i = 0; i < r; ++i) xl[i] = ldg_u8(p + tpos + i);
        nx = r;
      }
      if constexpr (kCopy) {
        if (dp)
          for (uint32_t i = 0; i < r; ++i) stg_u8(dp + tpos + i, ldg_u8(p + tpos + i));
      }
      len += go ? plen : 0;

      // ---- Sum on a copy
      uint32_t dig[5] = {0, 0, 0, 0, 0};
      if (go && fin && do_sha) {
        const uint32_t nxf = nx > 0 ? (uint32_t)nx : 0u;
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

      // ---- the member's sum, status and record (the state itself waits for the chain's end)
      if (go) {
        dirty = dirty || !keep;
        if (fin && jb.sum) {
#pragma unroll
          for (int k = 0; k < 5; ++k) reinterpret_cast<uint32_t*>(jb.sum)[k] = bswap(status == EFES_OK ? dig[k] : 0u);
          reinterpret_cast<uint32_t*>(jb.sum)[5] = bswap(do_crc ? ~crc_raw : 0u);
        }
      }
      if (valid && jb.status) *jb.status = go ? status : EFES_ERR_STATE;
      if (kCkpt && go && !keep) {
        uint32_t* ck = reinterpret_cast<uint32_t*>(ckpt[cur]);
        if (ck) {
          constexpr int kXWord = (int)(offsetof(efes_sha1_state, x) / 4);
          constexpr int kPadWord = (int)(offsetof(efes_sha1_state, _pad) / 4);
          constexpr int kNxWord = (int)(offsetof(efes_sha1_state, nx) / 4);
          constexpr int kLenWord = (int)(offsetof(efes_sha1_state, len) / 4);
          constexpr int kCrcWord = (int)(offsetof(efes_checkpoint, crc32) / 4);
          static_assert(kXWord == 5 && kPadWord == kXWord + 16 && kNxWord == kPadWord + 1 && kLenWord == kNxWord + 2 &&
                            kCrcWord == kLenWord + 2 && sizeof(efes_checkpoint) / 4 == kCrcWord + 2,
                        "the 28 words of a record");
#pragma unroll
          for (int k = 0; k < 5; ++k) ck[k] = do_sha ? h[k] : 0u;
#pragma unroll
          for (int k = 0; k < 16; ++k)
            ck[kXWord + k] = do_sha ? (uint32_t)xl[4 * k] | (uint32_t)xl[4 * k + 1] << 8 |
                                          (uint32_t)xl[4 * k + 2] << 16 | (uint32_t)xl[4 * k + 3] << 24
                                    : 0u;
          ck[kPadWord] = 0u;
          ck[kNxWord] = do_sha ? (uint32_t)(uint64_t)nx : 0u;
          ck[kNxWord + 1] = do_sha ? (uint32_t)((uint64_t)nx >> 32) : 0u;
          ck[kLenWord] = do_sha ? (uint32_t)len : 0u;
          ck[kLenWord + 1] = do_sha ? (uint32_t)(len >> 32) : 0u;
          ck[kCrcWord] = do_crc ? ~crc_raw : 0u;
          ck[kCrcWord + 1] = 0u;
        }
      }
      if (active) ++cur;
    }

    // ---- the chain's state, once (a Sum-only head leaves the states alone: Go's Sum works on a copy)
    if (dirty) {
      if (st) {
#pragma unroll
        for (int k = 0; k < 5; ++k) st->h[k] = h[k];
#pragma unroll
        for (int k = 0; k < 16; ++k)
          reinterpret_cast<uint32_t*>(st->x)[k] = (uint32_t)xl[4 * k] | (uint32_t)xl[4 * k + 1] << 8 |
                                                  (uint32_t)xl[4 * k + 2] << 16 | (uint32_t)xl[4 * k + 3] << 24;
        st->nx = nx;
        st->len = len;
      }
      if (cs) cs->crc = ~crc_raw;
    }
  }
  if (lane == 0) __atomic_store_n(&L.prog[wv], 0xffffffffu, __ATOMIC_RELAXED);  // done: never the slowest
