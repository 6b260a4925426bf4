/*
 * efes_hash.h -- C ABI of the MI355X-native content-hashing path of efes.
 *
 * This library replaces the per-chunk SHA-1 + CRC-32/IEEE that putdotio/efes streams
 * every uploaded byte through.  Cited reference interfaces (/root/reference/<file>:<line>):
 *   sha1digest  (sha1.go:29-120), its text codec (sha1_efes.go:25-64),
 *   crc32digest (crc32.go:48-93), its text codec (crc32_efes.go:18-40),
 *   and the hot loop io.MultiWriter(f, CRC32, Sha1) + io.Copy (filereceiver.go:208-209).
 *
 * Two layers:
 *   1. Batched device-resident hot path (efes_hash_submit): every job is ONE `Write(p)`
 *      (sha1.go:58-79 and crc32.go:76-86) of a device buffer into a device-resident
 *      state, optionally followed by `Sum` (sha1.go:82-120, crc32.go:90-93).  All
 *      compression runs in hand-written gfx950 kernels.  Jobs are independent.
 *   2. Streaming digest objects mirroring the Go `hash.Hash` surface (efes_sha1_*,
 *      efes_crc32_*), staging host bytes and hashing them on the GPU through layer 1.
 *      Their MarshalText/UnmarshalText are byte-identical to the reference's, so
 *      `<path>.info` files (fileinfo.go:10-58) stay interchangeable.
 *
 * Plain C types only; every pointer documented "device" must be device memory of the
 * context's GPU (hipMalloc), "host" pointers are ordinary host memory.  Functions
 * return 0 (EFES_OK) or a negative efes error code; nothing panics or aborts.
 * All functions are thread-safe except concurrent use of ONE streaming object.
 */
#ifndef EFES_HASH_H
#define EFES_HASH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EFES_ABI_VERSION 8

/* ---- error codes ---------------------------------------------------------------- */
#define EFES_OK 0
#define EFES_ERR_INVALID_DIGEST (-1) /* sha1_efes.go:23 errInvalidDigest (bad text length / hex) */
#define EFES_ERR_STATE (-2)          /* state on which the Go code would panic: nx > 64 at Write
                                        (slice bounds, sha1.go:62) or d.nx != 0 in checkSum (sha1.go:107-109) */
#define EFES_ERR_HIP (-3)            /* a HIP runtime call failed (device fault, OOM, ...) */
#define EFES_ERR_ARG (-4)            /* invalid argument (NULL, bad flags, misaligned state) */
#define EFES_ERR_NO_DEVICE (-5)      /* no usable gfx950 device */
#define EFES_ERR_NOMEM (-6)          /* host allocation failed */
#define EFES_ERR_DEVICE_FAULT (-7)   /* an earlier asynchronous device error was latched */

const char* efes_strerror(int code);
int efes_abi_version(void);
/* The identity of the sources the library was built from (ABI 7): 16 hex digits of a SHA-256 over its
 * source and header files, compiled in by efes_amd/build.py ("unversioned" for any other build), so a
 * deployment -- and the GPU tests -- can check that the loaded library matches the sources beside it. */
const char* efes_build_id(void);

/* ---- state layouts (device- and host-side identical) ----------------------------- */

/* sha1.go:29-34 `sha1digest`: field order = MarshalText order (sha1_efes.go:26-34). */
typedef struct efes_sha1_state {
    uint32_t h[5];  /* running hash */
    uint8_t x[64];  /* tail buffer; bytes x[nx:64] are stale, exactly as in Go */
    uint32_t _pad;  /* keeps nx/len 8-byte aligned; ignored */
    int64_t nx;     /* bytes pending in x (Go int) */
    uint64_t len;   /* total bytes written (Go uint64, wraps) */
} efes_sha1_state; /* 104 bytes */

/* crc32.go:48-51 `crc32digest` (the table is always IEEE, crc32_efes.go:37-38). */
typedef struct efes_crc32_state {
    uint32_t crc; /* the finalized CRC-32/IEEE of everything written so far (Sum32) */
} efes_crc32_state;

/* sha1.go:36-44 Reset / sha1.go:48-52 NewSha1. */
void efes_sha1_state_init(efes_sha1_state* s);

/* ---- context ----------------------------------------------------------------------- */
typedef struct efes_ctx efes_ctx;

/* HIP devices visible to the process, of any architecture (ABI 7): 0 when there are none or the
 * runtime fails.  A binding opens every ordinal below it and SKIPS the ones efes_ctx_create refuses
 * (EFES_ERR_NO_DEVICE for a non-gfx950 card, EFES_ERR_HIP / EFES_ERR_NOMEM for one that fails to
 * initialise), so one bad GPU does not hide the GPUs after it (go/hash_gpu.go pool()). */
int efes_device_count(void);
/* Binds one GPU (HIP device ordinal), uploads the CRC tables, creates a stream.  EFES_ERR_ARG for an
 * ordinal outside [0, efes_device_count()), EFES_ERR_NO_DEVICE for a device that is not gfx950. */
int efes_ctx_create(int device, efes_ctx** out);
void efes_ctx_destroy(efes_ctx* ctx);
int efes_ctx_device(const efes_ctx* ctx);
/* The context's own stream (a hipStream_t), used when a call passes stream == NULL. */
void* efes_ctx_stream(efes_ctx* ctx);

/* ---- layer 1: batched device-resident jobs ----------------------------------------- */
#define EFES_JOB_FINALIZE 0x1u /* also write Sum of the post-Write state to `sum` */
#define EFES_JOB_INIT 0x2u     /* start from NewSha1() / NewCRC32IEEE() (sha1.go:48-52, crc32.go:68):
                                  the in-states are not read, only written (a fresh chunk) */
#define EFES_JOB_SUM_ONLY 0x4u /* with EFES_JOB_FINALIZE and length 0: Sum of the in-state on a copy
                                  (sha1.go:82-87 `d0 := *d`): the states are read, never written, so
                                  a pending full tail (nx == 64) stays pending as in Go */
#define EFES_JOB_CHAIN 0x8u    /* efes_crc32_chain and efes_hash_chain(_mode) only: this job is the next Write into
                                  the state(s) of the job before it (below); every other call ignores the bit */

/* One `Write(p)` (+ optional Sum) of len(p) = length bytes at device address `data`.
 * sha1 / crc32: device states updated in place; either may be NULL to skip that hash
 * (the MultiWriter of filereceiver.go:208 passes both).  sum (device, 24 bytes, only
 * with EFES_JOB_FINALIZE): SHA-1 Sum (20 B, sha1.go:82-87) then CRC-32 Sum (4 B BE,
 * crc32.go:90-93).  status (device, may be NULL): EFES_OK or EFES_ERR_STATE.
 * Jobs in one submit must not share a state. */
typedef struct efes_job {
    const void* data;
    uint64_t length;
    efes_sha1_state* sha1;
    efes_crc32_state* crc32;
    uint8_t* sum;
    int32_t* status;
    uint32_t flags;
    uint32_t _reserved;
} efes_job; /* 56 bytes */

/* Kernel shapes: DEEP = one wavefront per job (few, long jobs: per-job latency bound);
 * WIDE = one lane per job (many jobs: throughput bound).  AUTO picks by njobs.
 * GROUPn = grouped DEEP, 64/n jobs per wavefront with n lanes (n consecutive 64-B blocks
 * per step) each: for more long jobs than SIMDs (lower per-job latency than WIDE, fewer
 * instructions per byte than DEEP).  Jobs should be longest-first (efes_plan_batch).
 * AUTO picks by njobs (efes_auto_mode). */
#define EFES_MODE_AUTO 0
#define EFES_MODE_DEEP 1
#define EFES_MODE_WIDE 2
#define EFES_MODE_GROUP4 3
#define EFES_MODE_GROUP8 4
#define EFES_MODE_GROUP16 5
#define EFES_MODE_GROUP32 6
/* FED4: grouped DEEP (16 jobs of 4 lanes per chain wave) whose loads, CRC and schedule
 * expansion run on a producer wave on another SIMD of the same CU, so a job advances at DEEP's
 * per-block latency; 48 jobs per workgroup, each workgroup owns its CU.  For the longest jobs of
 * a mixed batch (efes_plan_batch), more of them than SIMDs. */
#define EFES_MODE_FED4 7
/* FED4E: FED4 with three chain waves and one producer per CU; the chain waves expand the
 * schedule themselves (the producer loads, CRCs and hands over the 16 message words): 48 jobs per
 * CU at a per-job latency between FED4's and GROUP4's. */
#define EFES_MODE_FED4E 8

/* Largest job count of one submit / plan / host batch (larger counts: EFES_ERR_ARG; split the
 * batch).  Keeps every grid size and lane index of the kernels within 32 bits. */
#define EFES_MAX_JOBS (1u << 30)

/* Enqueue njobs jobs (the job array itself in DEVICE memory) on `stream` (a
 * hipStream_t; NULL = the context stream).  Asynchronous; returns launch errors only. */
int efes_hash_submit(efes_ctx* ctx, const efes_job* jobs_device, uint32_t njobs, void* stream);
int efes_hash_submit_mode(efes_ctx* ctx, const efes_job* jobs_device, uint32_t njobs, void* stream, int mode);
/* The shape EFES_MODE_AUTO picks for njobs jobs of similar length (ctx may be NULL: one
 * MI355X): DEEP up to one job per SIMD, FED4 up to 32 per CU, FED4E up to 48 per CU, GROUP4 up to
 * 16 per SIMD (one wave each), WIDE beyond. */
int efes_auto_mode(const efes_ctx* ctx, uint32_t njobs);
/* Mixed-length batches (BASELINE configs[3], concurrent uploads of different sizes): the
 * makespan is set by the longest jobs (a SHA-1 chain per job), so a batch is cut, longest
 * first, into up to EFES_PLAN_MAX_PARTS consecutive parts that run CONCURRENTLY, each in its
 * own kernel shape: typically the longest jobs grouped-DEEP on CUs of their own (`exclusive`:
 * the launch reserves the CU's LDS so no other workgroup shares its SIMDs), the next ones
 * grouped-DEEP beside the rest, which run WIDE.
 * efes_plan_batch orders the jobs longest-first (order[i] = index into `lengths` of the job to
 * place at jobs_device[i]) and picks the cuts, shapes and exclusivity from an issue-time model
 * of the kernels calibrated on MI355X (DESIGN_NOTES.md §4); efes_hash_submit_plan launches a batch
 * laid out in that order: each part on a part stream of its own (created one after the other, so
 * usually -- HIP assigns hardware queues round-robin over all streams of the process, so not
 * certainly -- on distinct hardware queues), after the work queued on `stream`, which then waits
 * for all of them.  Planning is host-only (no device access; ctx
 * may be NULL: then the capacity of one MI355X, 256 CUs, is assumed). */
#define EFES_PLAN_MAX_PARTS 4
typedef struct efes_plan_part {
    uint32_t jobs;       /* consecutive jobs of this part (in plan order) */
    int32_t mode;        /* EFES_MODE_DEEP, EFES_MODE_GROUPn, EFES_MODE_FED4, EFES_MODE_FED4E or EFES_MODE_WIDE */
    uint32_t exclusive;  /* 1: each workgroup reserves its CU (one wave per SIMD); FED4/FED4E parts
                            ignore it: their workgroups always own their CU */
    uint32_t _reserved;
} efes_plan_part;
typedef struct efes_plan {
    uint32_t njobs;      /* jobs in the batch = sum of part[i].jobs */
    uint32_t nparts;     /* parts in use, 1..EFES_PLAN_MAX_PARTS (0 for an empty batch) */
    efes_plan_part part[EFES_PLAN_MAX_PARTS];
    double est_seconds;  /* the model's makespan estimate (informational) */
} efes_plan;
int efes_plan_batch(efes_ctx* ctx, const uint64_t* lengths, uint32_t n, uint32_t* order, efes_plan* plan);
int efes_hash_submit_plan(efes_ctx* ctx, const efes_job* jobs_device, const efes_plan* plan, void* stream);

/* Wait for `stream` (NULL = context stream); reports latched asynchronous errors. */
int efes_sync(efes_ctx* ctx, void* stream);

/* Device memory helpers for hosts without their own allocator (cgo). */
int efes_device_alloc(efes_ctx* ctx, size_t bytes, void** out);
int efes_device_free(efes_ctx* ctx, void* p);
int efes_copy_to_device(efes_ctx* ctx, void* dst_device, const void* src_host, size_t bytes, void* stream);
int efes_copy_to_host(efes_ctx* ctx, void* dst_host, const void* src_device, size_t bytes, void* stream);
/* Synthetic benchmark bytes: little-endian splitmix64 stream, z_i = mix(seed + (i+1)*0x9E3779B97F4A7C15). */
int efes_fill_synthetic(efes_ctx* ctx, void* dst_device, size_t bytes, uint64_t seed, void* stream);

/* ---- host-resident ingest -------------------------------------------------------------
 * The reference's path starts in host memory (a socket buffer, filereceiver.go:208-209).
 * efes_hash_host runs the jobs of a HOST array whose data/sha1/crc32/sum/status pointers are
 * all HOST memory: segment s (segment_bytes, rounded up to 64; 0 = 256 KiB) of every message is
 * copied H2D with hipMemcpyAsync on the context's copy stream (a hardware queue of its own) into
 * one of two device slots while segment s-1 is hashed on the context stream; concurrent calls on
 * one context take the copy stream in turn; states stay on the device between segments (the
 * per-PATCH resume of filereceiver.go:182-226); states, sums and status are copied back at
 * the end.  Equivalent to one Write per segment (so the stale bytes x[nx:64] are those of
 * segment-sized Writes, sha1.go:75-77).  Messages whose host addresses advance by a constant stride are copied with one
 * 2D copy per segment.  For the full PCIe rate the data should be pinned (efes_host_alloc).
 * Synchronous; stats (may be NULL) time the pipeline from the first copy to the last result. */
/* segment_bytes == EFES_HOST_ZERO_COPY: every data pointer is pinned, device-mapped host memory
 * (efes_host_alloc) and one launch reads it in place over PCIe: no staging copies, no segments
 * (EFES_ERR_ARG if a pointer is not device-accessible).  Stats time the launch and the result
 * copies. */
#define EFES_HOST_ZERO_COPY ((uint64_t)-1)
typedef struct efes_host_stats {
    double seconds;    /* wall time of the copy+hash pipeline */
    uint64_t bytes;    /* message bytes moved and hashed */
    uint32_t segments; /* pipeline steps */
    uint32_t _reserved;
} efes_host_stats;

int efes_hash_host(efes_ctx* ctx, const efes_job* jobs_host, uint32_t njobs, uint64_t segment_bytes,
                   efes_host_stats* stats);
int efes_host_alloc(efes_ctx* ctx, size_t bytes, void** out); /* pinned, device-mapped host memory */
int efes_host_free(efes_ctx* ctx, void* p);

/* ---- concurrent uploads: batching dispatcher ------------------------------------------
 * An efes_upload is the MultiWriter(CRC32, Sha1) of ONE upload (filereceiver.go:208) with
 * both states in HBM.  efes_upload_write copies into pinned staging (chunk_bytes pieces out
 * of max_chunks; it blocks only when all are in use) and returns; the queue's dispatcher
 * thread launches the staged chunks of ALL uploads together -- one job per upload per launch,
 * so each upload's chain stays in order -- while callers keep staging.  Sync points wait for
 * that upload's bytes only: flush; state (h/crc from the device, x/nx/len replayed on the host
 * per Write, so MarshalText of it is byte-identical to Go's after the same Writes); sum
 * (SHA-1 Sum || CRC Sum, non-destructive, sha1.go:82-87).  Uploads may be used from different
 * threads concurrently; one upload must not be written from two threads at once (each Go
 * digest belongs to one request goroutine, server.go:130).  max_uploads bounds open uploads
 * and must be < max_chunks (each open upload may hold one partly filled chunk). */
typedef struct efes_queue efes_queue;
typedef struct efes_upload efes_upload;
#define EFES_HASH_SHA1 0x1u  /* which digests an upload keeps (a MultiWriter of both is 0x3) */
#define EFES_HASH_CRC32 0x2u
int efes_queue_create(efes_ctx* ctx, uint64_t chunk_bytes, uint32_t max_chunks, uint32_t max_uploads,
                      efes_queue** out);
void efes_queue_destroy(efes_queue* q); /* finishes launched work; close uploads first */
/* hashes: EFES_HASH_SHA1 | EFES_HASH_CRC32; sha1 / crc32: initial states (host), NULL =
 * NewSha1() / NewCRC32IEEE().  Sums of a digest the upload does not keep read as zeros. */
int efes_upload_open(efes_queue* q, uint32_t hashes, const efes_sha1_state* sha1, const efes_crc32_state* crc32,
                     efes_upload** out);
int efes_upload_write(efes_upload* u, const void* p, size_t n);
/* Zero-copy staging (ABI 3): *p / *n = at least min(min_bytes, chunk_bytes) contiguous bytes of
 * the upload's pinned staging chunk (a partly filled chunk with less room is handed to the
 * dispatcher first; blocks while every chunk is in use).  Fill k <= *n of them -- read a request
 * body straight in, write the file from there -- and efes_upload_commit(u, k): the same as
 * efes_upload_write of those k bytes (one Write of k bytes, sha1.go:58-79) without the copy.
 * Bytes reserved but not committed are dropped; reserve again before the next commit (a commit
 * of more bytes than the last reserve granted, a second commit, or a commit after a write returns
 * EFES_ERR_ARG).  The pointer is valid only until the commit. */
int efes_upload_reserve(efes_upload* u, size_t min_bytes, void** p, size_t* n);
int efes_upload_commit(efes_upload* u, size_t k);
int efes_upload_flush(efes_upload* u);
int efes_upload_state(efes_upload* u, efes_sha1_state* sha1, efes_crc32_state* crc32);
int efes_upload_sum(efes_upload* u, uint8_t out[24]);
void efes_upload_close(efes_upload* u); /* drops bytes staged since the last sync point */
/* Counters of a queue (ABI 5): what its dispatcher launched, and its upload slots. */
typedef struct efes_queue_stats {
    uint64_t launches;      /* kernel launches */
    uint64_t jobs;          /* jobs in them (one per upload per launch, Sums included) */
    uint64_t bytes;         /* staged bytes hashed */
    uint32_t free_uploads;  /* upload (state) slots free now */
    uint32_t max_uploads;
} efes_queue_stats;
int efes_queue_get_stats(efes_queue* q, efes_queue_stats* out);

/* ---- layer 2: streaming digests mirroring the Go surface ----------------------------
 * Each object is an upload (above) of the context's shared digest queue that keeps only its
 * own hash, so unchanged Go code -- MultiWriter(f, CRC32, Sha1) in every request goroutine --
 * is batched across all concurrent requests: Write stages into pinned memory and returns,
 * Sum / Sum32 / MarshalText are the sync points.  The shared queue holds
 * EFES_DIGEST_STAGING_MIB (env, default 1024) of pinned staging in EFES_DIGEST_CHUNK_KIB (default
 * 256) chunks and EFES_DIGEST_SLOTS (default 65536) upload slots: a digest (a fused CRC + SHA-1 pair
 * is one) holds a slot from its first Write to its sync point; when writers wait for a chunk and
 * every chunk sits partly filled in idle uploads, the queue's dispatcher has those handed over.  A
 * Write blocks while all chunks are in flight.  EFES_DIGEST_SLOTS below the chunk count gives one
 * slot per chunk at most (no hand-over; a Write evicts instead, below).
 *
 * Go's Write never fails (sha1.go:58-79, crc32.go:76-86), and neither does this one for any
 * number of live digests:
 *   - a digest holds an upload slot only between its first Write and its next sync point: every
 *     Sum / Sum32 / MarshalText parks the state on the host and gives the slot back, the next
 *     Write takes one again (so digests that are never freed hold no queue resources);
 *   - a Write (or Sum) that finds every slot taken waits for a holder's sync point; it evicts the
 *     oldest holder that is not inside a call and has been idle for EFES_DIGEST_EVICT_MS (env,
 *     default 50; a stalled client, an abandoned digest) -- or, once it has itself waited that
 *     long, the oldest holder not inside a call -- hashing what that one staged and parking its
 *     state on the host; back-pressure, never EFES_ERR_NOMEM;
 *   - a device or HIP fault during a Write is latched and the Write returns EFES_OK: the next
 *     Sum / Sum32 / MarshalText reports it (MarshalText's error -> HTTP 500, filereceiver.go:94-96).
 * Write returns an error only for bad arguments and for the states on which Go's Write panics
 * (EFES_ERR_STATE: nx > 64, sha1.go:62).  The object itself is host memory, so freeing it late
 * (a Go finalizer) costs nothing scarce. */
typedef struct efes_sha1 efes_sha1;
typedef struct efes_crc32 efes_crc32;

/* Fused pairs (ABI 6).  io.MultiWriter(f, CRC32, Sha1) (filereceiver.go:208-209) hands every body
 * buffer to the CRC digest and then, unchanged, to the SHA-1 digest.  The library detects that
 * pattern and binds the two digests to ONE upload keeping both hashes, so each byte is staged once
 * and hashed by one fused job, as efes_upload_* does for a caller that asks for it:
 *   - a CRC digest's first Write after a sync point is held back (copied) as a candidate; a parked
 *     SHA-1 digest's Write with the same pointer and length binds to it, and the pair opens one
 *     upload (a candidate nobody binds is staged at the CRC digest's next call);
 *   - then each CRC Write is held back until the SHA-1 Write of the same (p, n) -- of any size --
 *     is staged and compared with it in one pass, which confirms it;
 *   - anything else (a Write to one digest only, other bytes, the CRC digest synced first, Reset /
 *     UnmarshalText / free of one, an eviction) splits the pair: every confirmed byte is in both
 *     states, an unconfirmed CRC Write in the CRC state only, and both go on alone.
 * Every digest therefore hashes exactly the bytes of its own Writes, in order, whatever the caller
 * does; only the speed depends on the pattern.  Process-wide counters: */
typedef struct efes_pair_stats {
    uint64_t pairs;         /* CRC + SHA-1 digests bound to one upload */
    uint64_t fused_writes;  /* SHA-1 Writes confirming the CRC Write (one staging copy, one job) */
    uint64_t fused_bytes;   /* their bytes */
    uint64_t settles;       /* pairs split (diverging Writes, evictions) */
} efes_pair_stats;
int efes_pair_stats_get(efes_pair_stats* out);

int efes_sha1_new(efes_ctx* ctx, efes_sha1** out);                       /* sha1.go:48-52 NewSha1 */
int efes_sha1_new_zero(efes_ctx* ctx, efes_sha1** out);                  /* `var d sha1digest` (zero value) */
void efes_sha1_free(efes_sha1* d);
void efes_sha1_reset(efes_sha1* d);                                      /* sha1.go:36-44 */
int efes_sha1_size(void);                                                /* sha1.go:54 (20) */
int efes_sha1_block_size(void);                                          /* sha1.go:56 (64) */
int efes_sha1_write(efes_sha1* d, const void* p, size_t n);              /* sha1.go:58-79 */
int efes_sha1_sum(efes_sha1* d, uint8_t out[20]);                        /* sha1.go:82-87 */
int efes_sha1_marshal_text(efes_sha1* d, char out[200]);                 /* sha1_efes.go:25-38 */
int efes_sha1_unmarshal_text(efes_sha1* d, const char* text, size_t n);  /* sha1_efes.go:40-64 */
int efes_sha1_get_state(efes_sha1* d, efes_sha1_state* out);
int efes_sha1_set_state(efes_sha1* d, const efes_sha1_state* in);

int efes_crc32_new(efes_ctx* ctx, efes_crc32** out);                     /* crc32.go:68 NewCRC32IEEE */

/* Multi-GPU digests (ABI 5).  A storage server is one process (server.go:130, one goroutine per
 * request), so one process's digests should use every GPU: a pool spreads them over its
 * contexts.  A pooled digest takes its upload slot, at every (re)open, on the context whose digest
 * queue has the most free slots (its state is on the host between sync points, so consecutive
 * PATCHes of one object may run on different GPUs; the byte order is kept by the caller).  The
 * contexts must outlive the pool, and the pool its digests. */
typedef struct efes_pool efes_pool;
int efes_pool_create(efes_ctx* const* ctxs, uint32_t n, efes_pool** out);
void efes_pool_destroy(efes_pool* p);
int efes_sha1_new_pool(efes_pool* p, efes_sha1** out);                   /* NewSha1 on the pool */
int efes_sha1_new_zero_pool(efes_pool* p, efes_sha1** out);              /* `var d sha1digest` on the pool */
int efes_crc32_new_pool(efes_pool* p, efes_crc32** out);                 /* NewCRC32IEEE on the pool */
/* Counters of the digest queue of the pool's i-th context (zeros before its first digest Write). */
int efes_pool_stats(efes_pool* p, uint32_t i, efes_queue_stats* out);
void efes_crc32_free(efes_crc32* d);
void efes_crc32_reset(efes_crc32* d);                                    /* crc32.go:74 */
int efes_crc32_size(void);                                               /* crc32.go:70 (4) */
int efes_crc32_block_size(void);                                         /* crc32.go:72 (1) */
int efes_crc32_write(efes_crc32* d, const void* p, size_t n);            /* crc32.go:76-86 */
int efes_crc32_sum32(efes_crc32* d, uint32_t* out);                      /* crc32.go:88 */
int efes_crc32_sum(efes_crc32* d, uint8_t out[4]);                       /* crc32.go:90-93 */
int efes_crc32_marshal_text(efes_crc32* d, char out[8]);                 /* crc32_efes.go:18-24 */
int efes_crc32_unmarshal_text(efes_crc32* d, const char* text, size_t n);/* crc32_efes.go:26-40 */

/* Host-side diagnostics (no device work): copies the CRC-32 tables the kernels use,
 * slice8[8][256] (crc32.go:138-149) then shift[7][4][256] (advance of the raw register
 * over 64<<k zero bytes, byte-sliced), then -- when nwords leaves room for them (9216 + 16384
 * words) -- the position tables pos[64][256] (the raw register after a 64-byte block whose only
 * nonzero byte is b at offset o, from register 0: the WIDE and grouped kernels' block CRC);
 * returns the word count written or EFES_ERR_ARG. */
int efes_crc32_tables(uint32_t* out, size_t nwords);

/* CRC-32 of A||B from crc(A), crc(B) and |B| (crc32.go is GF(2)-linear: the zlib
 * crc32_combine identity), so chunks of one object can be CRC'd out of order or on different
 * devices and merged on the host; len2 may be any size (O(log len2) 32x32 GF(2) products). */
uint32_t efes_crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2);

/* CRC-32 of ONE long device buffer on the whole GPU: the same result as
 * crc32.go's Write (76-86) of `length` bytes at `data` (device memory, any alignment) into the
 * device state *crc -- so chained calls compose like Writes and efes_crc32_combine merges pieces
 * hashed on different GPUs -- but computed segment-parallel instead of byte by byte: every 64-byte
 * block's raw CRC from position tables, merged by the GF(2)-linearity that efes_crc32_combine uses.
 * For an object's CRC alone (a re-check after a copy or drain); uploads keep the fused SHA-1 +
 * CRC-32 jobs above, whose speed SHA-1's serial chain sets.  Asynchronous on `stream` (NULL = the
 * context stream); calls that share a state must be ordered on one stream. */
int efes_crc32_span(efes_ctx* ctx, const void* data_device, uint64_t length, efes_crc32_state* crc_device,
                    void* stream);

/* CRC-32 of MANY device buffers in one call (ABI 8): njobs efes_job records in device memory, exactly
 * as for efes_hash_submit, each with sha1 == NULL.  For every such job the call writes what
 * efes_hash_submit writes for it -- crc32->crc, the 24-byte sum under EFES_JOB_FINALIZE (20 zero
 * bytes, then the CRC big-endian), status; EFES_JOB_INIT and EFES_JOB_SUM_ONLY as above; crc32 == NULL
 * hashes nothing; any data alignment, any length -- but the bytes of ALL jobs are cut into tiles of
 * EFES_CRC_BATCH_TILE bytes that are dealt evenly to the whole GPU, so a few long buffers, or long and
 * short ones mixed, take the time of their total size, not of the longest job on one wavefront.  A
 * job with sha1 != NULL gets status EFES_ERR_ARG and nothing else of it is written; its neighbours
 * are unaffected.  Jobs of one call must not share a state.  The lengths are read on the device:
 * the host reads back nothing, allocates nothing and waits for nothing.  Asynchronous on `stream`
 * (NULL = the context stream).
 * scratch_device: device memory of the context's GPU, 16-byte aligned, at least
 * efes_crc32_batch_scratch(njobs) bytes (0 for njobs == 0 or > EFES_CRC_BATCH_MAX_JOBS), used in stream
 * order from the call until its work is done: calls that may overlap (different streams) need a
 * scratch buffer each; calls on one stream may share one.
 * Returns EFES_ERR_ARG for a NULL ctx, NULL jobs with njobs > 0, njobs > EFES_CRC_BATCH_MAX_JOBS (split
 * the batch), and scratch that is NULL, too small or misaligned; njobs == 0 returns EFES_OK and
 * launches nothing.
 * Which CRC path when (measured on 4 GiB per shape, profiles/crc_batch/bench.json; DESIGN.md §4
 * "Batched CRC" has the table):
 *   - ONE long buffer: efes_crc32_span.  Its LDS-DMA reads stay ahead: the batch call reads the same
 *     4 GiB object at about 0.85 of the span's rate;
 *   - two or more buffers of 1 MiB and up, of equal or of mixed sizes (objects re-checked after a copy
 *     or drain, the pieces of shard.py): efes_crc32_batch.  It holds about 0.7 of the 8 TB/s spec from
 *     16 x 256 MiB down to 1024 x 4 MiB, where CRC-only jobs of efes_hash_submit give each buffer one
 *     wavefront and run 150x (16 buffers) to 2.5x (1024) slower, and one span call per buffer takes
 *     1.1x (16 buffers) to 1.8x (64) as long;
 *   - very many small buffers (65 536 x 64 KiB: one tile per job): CRC-only jobs of efes_hash_submit,
 *     whose WIDE shape hashes one buffer per lane at about twice the batch call's rate there (the
 *     batch call ends a run, with a workgroup barrier, at every tile);
 *   - CRC jobs mixed with SHA-1 jobs in one array: efes_hash_submit (the batch call refuses them). */
#define EFES_CRC_BATCH_TILE 65536u
#define EFES_CRC_BATCH_MAX_JOBS (1u << 20)
size_t efes_crc32_batch_scratch(uint32_t njobs);
int efes_crc32_batch(efes_ctx* ctx, const efes_job* jobs_device, uint32_t njobs, void* scratch_device,
                     size_t scratch_bytes, void* stream);

/* Chained CRC jobs: ONE object in MANY device extents (PATCH-sized chunks, staging chunks, the pieces
 * of shard.py, extents of a buffer pool).  efes_crc32_chain is efes_crc32_batch -- the same device job
 * array, lengths read on the device, no host read-back, allocation or wait, asynchronous on `stream`,
 * the same argument errors, njobs <= EFES_CRC_BATCH_MAX_JOBS, njobs == 0 returns EFES_OK and launches
 * nothing, the same scratch rules with efes_crc32_chain_scratch(njobs) bytes (>= the batch call's) --
 * that also honours EFES_JOB_CHAIN:
 *   - a chain is a head job (flag clear) and the consecutive jobs behind it that carry the flag; its
 *     members are Write(p0); Write(p1); ... (crc32.go:76-86) into the one state they all name.  An
 *     unflagged job is a chain of one: for an array without the flag the call writes byte for byte what
 *     efes_crc32_batch writes.  Chains of one call must not share a state with each other;
 *   - the head may carry EFES_JOB_INIT, or starts from the state's value;
 *   - every member with EFES_JOB_FINALIZE gets its own 24-byte sum: 20 zero bytes, then the CRC after
 *     THAT member's Write, big-endian -- the running CRC of the object at that extent's end, what
 *     `.info` holds after each PATCH (fileinfo.go:10-58).  A zero-length FINALIZE member gives the sum
 *     EFES_JOB_SUM_ONLY would;
 *   - crc32->crc is written once, by the chain's last valid member, with the CRC after its Write;
 *   - every member gets a status;
 *   - a flagged job is invalid when it is job 0, has sha1 != NULL or crc32 == NULL, names another state
 *     than the job before it, also carries EFES_JOB_INIT or EFES_JOB_SUM_ONLY, follows an
 *     EFES_JOB_SUM_ONLY job, or follows an invalid member of its chain; a head with sha1 != NULL is
 *     invalid as in the batch call.  An invalid member gets status EFES_ERR_ARG and nothing else of it
 *     is written (its data bytes may be read).  The valid members before it have taken effect, as the
 *     Writes before a panicking Write have in Go; the next chain is unaffected.
 * The extents are dealt to the GPU exactly as the same extents would be as separate jobs of
 * efes_crc32_batch; the Writes are then composed on the device as affine maps of the CRC register by a
 * parallel prefix scan (DESIGN.md §4 "Chained CRC").
 * Other calls: efes_crc32_batch and the efes_hash_submit family ignore EFES_JOB_CHAIN as they ignore
 * every unknown bit, so there the flagged jobs are independent jobs and "jobs in one submit must not
 * share a state" still holds; efes_hash_host rejects unknown flags.  EFES_ABI_VERSION stays 8: the
 * addition changes nothing that existed, and a binding detects it by the symbol.
 * Which CRC path when, continued (measured on 4 GiB per shape, profiles/crc_chain/bench.json; DESIGN.md
 * §4 "Chained CRC" has the table):
 *   - objects that lie in several extents each (64 objects x 64 extents x 1 MiB and 1024 objects x 64
 *     extents x 64 KiB measured): efes_crc32_chain.  On the device it takes the time of efes_crc32_batch
 *     over the same extents as separate jobs, within 5 % either way, and the object CRCs (and the CRC
 *     after every extent, where asked) are ready on the device.  efes_crc32_batch into piece states,
 *     then a copy of the piece CRCs to the host and efes_crc32_combine per piece there, has the object
 *     CRCs on the host about 15x (4096 extents) to 100x (65 536 extents) later, the fold measured through
 *     the Python binding; one efes_crc32_span per extent on one stream takes about 70x to 400x as long;
 *   - an array without EFES_JOB_CHAIN: either call; efes_crc32_batch is some 30 us (4 % of 4 GiB at
 *     1024 x 4 MiB) shorter, the cost of scanning instead of one finish launch. */
size_t efes_crc32_chain_scratch(uint32_t njobs);
int efes_crc32_chain(efes_ctx* ctx, const efes_job* jobs_device, uint32_t njobs, void* scratch_device,
                     size_t scratch_bytes, void* stream);

/* Copy with CRC: move device extents and CRC them in ONE pass over their bytes -- io.MultiWriter(f, CRC32)
 * with a device destination as the first writer (filereceiver.go:208-209): gather an object's extents
 * into one contiguous buffer before a write-out, compact a pool, move a drained object.
 * efes_crc32_copy is efes_crc32_chain plus a copy of each job's bytes.  Everything of the chain call
 * carries over: the same device job array, EFES_JOB_CHAIN / INIT / FINALIZE / SUM_ONLY, every validity
 * rule, status, state store and per-member sum, lengths read on the device, no host read-back,
 * allocation or wait, asynchronous on `stream`, njobs <= EFES_CRC_BATCH_MAX_JOBS, njobs == 0 returns
 * EFES_OK and launches nothing, the same scratch rules with efes_crc32_copy_scratch(njobs) bytes (>=
 * efes_crc32_chain_scratch(njobs), 0 where that is 0).  On any job array everything efes_crc32_chain
 * writes is written byte for byte the same.  The copy:
 *   - dst_device is a device array of njobs device pointers, parallel to jobs_device.  dst[j] may have
 *     any alignment, independent of the alignment of jobs[j].data; dst[j] == NULL: job j is hashed and
 *     not copied.  A NULL dst_device with njobs > 0 returns EFES_ERR_ARG: use efes_crc32_chain;
 *   - a valid job's `length` bytes are written to [dst[j], dst[j] + length), exactly.  No byte outside
 *     that range is written for any job, valid or not; a zero-length job writes nothing;
 *   - a job with sha1 != NULL or crc32 == NULL is not read, and nothing is copied for it;
 *   - a chain member that is invalid for any other reason (it names another state, carries
 *     EFES_JOB_INIT or EFES_JOB_SUM_ONLY, follows an EFES_JOB_SUM_ONLY job or an invalid member, or is a
 *     flagged job 0) may or may not have had its bytes written: after the call every byte of its
 *     destination range holds either its old value or the source byte, unspecified which -- chain
 *     validity is known only after the scan, which runs behind the pass that moves the bytes.  Its
 *     status and everything else are as in the chain call;
 *   - destination ranges must not overlap each other, nor any job's source range, the states, sums,
 *     statuses, the job array, the pointer array or the scratch.  Like "jobs must not share a state"
 *     this is the caller's contract and is not checked;
 *   - the destination bytes are visible to later work in stream order, like the states.
 * The tile pass that hashes a job's 16-byte pieces stores each piece from the registers it was loaded
 * into (one plain 16-byte store per piece, at whatever alignment the destination has); the scan's map
 * pass lands the up to 15 bytes before and behind the pieces.  EFES_ABI_VERSION stays 8: the call is an addition, and a binding detects
 * it by the symbol.
 * Which path when, continued (measured on a 4 GiB source and a 4 GiB destination per shape,
 * profiles/crc_copy/bench.json; DESIGN.md §4 "Copy with CRC" has the table):
 *   - extents that have to be moved AND checked (gather before a write-out, pool compaction, a drained
 *     object's move): efes_crc32_copy.  The yardstick is the best single-launch copy (one memcpy for
 *     16 x 256 MiB, one strided copy in 16-byte elements for the transposing gathers) followed by
 *     efes_crc32_chain over the source.  The call takes about 0.7 of that time at 16 x 256 MiB and at
 *     64 objects x 64 extents x 1 MiB and about 0.6 at 1024 objects x 64 extents x 64 KiB, its median
 *     below the two-call path's minimum on all three: the second read of the bytes is gone, as the
 *     traffic says (two thirds).  It moves 4.5 to 5.1 TB/s (read + written) and takes at most 1.25x the
 *     time of the copy ALONE: the CRC rides along on a move that has to happen anyway;
 *   - relative misalignment (destination + 1 byte or + 8 bytes against a 16-byte aligned source) costs
 *     the call under 2 %, so no layout needs padding for it.  A strided copy loses its wide elements
 *     there (single bytes at + 1: 3.3x its aligned time), which makes the call the faster MOVE for such
 *     layouts, CRC or not;
 *   - extents that are only checked, or that are moved by something that cannot hash (a DMA engine,
 *     another GPU's copy): efes_crc32_chain, which reads the same bytes at about 5.6 TB/s and writes
 *     nothing. */
size_t efes_crc32_copy_scratch(uint32_t njobs);
int efes_crc32_copy(efes_ctx* ctx, const efes_job* jobs_device, void* const* dst_device, uint32_t njobs,
                    void* scratch_device, size_t scratch_bytes, void* stream);

/* Chained SHA-1 + CRC-32 jobs: efes_hash_submit for objects that lie in MANY device extents.  The same
 * device job array as efes_hash_submit, fused, SHA-1-only or CRC-only jobs, lengths and flags read on
 * the device, no host read-back, allocation or wait, asynchronous on `stream` (NULL = the context
 * stream); njobs <= EFES_HASH_CHAIN_MAX_JOBS.  The call honours EFES_JOB_CHAIN, and its yardstick is Go's
 * Write; Write; ... into one digest pair: what njobs successive efes_hash_submit_mode(EFES_MODE_DEEP)
 * calls of one job each, on one stream, would leave behind.
 *   - a chain is a head job (flag clear) and the consecutive jobs behind it that carry the flag; its
 *     members are successive Writes into the one sha1 and/or crc32 state they all name (either pointer
 *     may be NULL for the whole chain).  Chains of one call must not share a state with each other;
 *   - the head takes every flag efes_hash_submit knows (EFES_JOB_INIT, EFES_JOB_FINALIZE,
 *     EFES_JOB_SUM_ONLY).  An unflagged job is a chain of one: for an array without the flag the call
 *     writes byte for byte what efes_hash_submit_mode(EFES_MODE_DEEP) writes -- the states with their
 *     stale bytes x[nx:64], the sums, the statuses;
 *   - every member with EFES_JOB_FINALIZE gets its own 24-byte sum from the state after THAT member's
 *     Write: SHA-1 Sum on a copy (sha1.go:82-87), then the CRC big-endian -- the running digest of the
 *     object at that extent's end.  For the CRC that is what `.info` holds after each PATCH
 *     (fileinfo.go:10-58), since its state is its sum; for SHA-1 `.info` holds the marshalled STATE
 *     (sha1_efes.go:25-38), which a 20-byte Sum cannot be resumed from: efes_hash_chain_checkpoints
 *     (below) leaves that state after every member.  Members of length zero are allowed;
 *   - after the call the states hold what they hold after the valid members' Writes in order (h, x
 *     with its stale bytes, nx, len, crc); whether intermediate values are stored on the way is
 *     unspecified;
 *   - every member gets a status.  EFES_ERR_STATE arises where the job kernels raise it: with nx > 64
 *     at a Write (sha1.go:62) that member writes nothing else, and the members behind it find the same
 *     state and get the same status, as successive Writes would; d.nx != 0 at Sum (sha1.go:107-109)
 *     gives EFES_ERR_STATE with the state written;
 *   - a flagged job is invalid when it is job 0, names a sha1 or a crc32 pointer other than the job
 *     before it, has both pointers NULL, also carries EFES_JOB_INIT or EFES_JOB_SUM_ONLY, follows an
 *     EFES_JOB_SUM_ONLY job, or follows an invalid member of its chain.  An invalid member gets status
 *     EFES_ERR_ARG and nothing else of it is written.  The valid members before it have taken effect;
 *     the next chain is unaffected.
 * scratch_device: device memory of the context's GPU, 16-byte aligned, at least
 * efes_hash_chain_scratch(njobs) bytes (0 for njobs == 0 or > EFES_HASH_CHAIN_MAX_JOBS), used in stream
 * order from the call until its work is done: calls that may overlap (different streams) need a
 * scratch buffer each; calls on one stream may share one.
 * Returns EFES_ERR_ARG for a NULL ctx, NULL jobs with njobs > 0, njobs > EFES_HASH_CHAIN_MAX_JOBS (split
 * the array between chains), and scratch that is NULL, too small or misaligned; njobs == 0 returns
 * EFES_OK and launches nothing.
 * The chains are found on the device (two small launches list the heads); then every wavefront of a
 * persistent launch draws whole chains and runs their members in order on the one-wave path of the
 * DEEP shape, so a call lasts as long as its longest chains, not as the sum over extent steps of the
 * longest extent in each (DESIGN.md §4 "Chained SHA-1 + CRC").  EFES_ABI_VERSION stays 8: the addition
 * changes nothing that existed, and a binding detects it by the symbol.
 * Which path when (measured, profiles/hash_chain_group/bench.json; DESIGN.md §4 "Chained SHA-1 + CRC,
 * grouped walk" has the table; "steps" = one efes_hash_submit per extent step on one stream, one job per
 * object that still has an extent, AUTO or forced DEEP; "grouped walk" = efes_hash_chain_mode at the mode
 * efes_hash_chain_auto_mode gives for the object count, declared below):
 *   - objects of UNEQUAL extent counts or sizes, no more of them than SIMDs (1024 objects of 1-64 extents
 *     of 4 KiB-1 MiB, longest first): efes_hash_chain.  It takes about 0.6 of the steps' device time: the
 *     longest object's own chain instead of the sum over steps of the longest extent in each;
 *   - objects of EQUAL extents, no more of them than SIMDs (1024 objects x 16 x 256 KiB, x 128 x 32 KiB):
 *     either.  On the device the chain call takes 3 to 4 % and 2 % longer than the steps -- its waves
 *     run without DEEP's producer wave -- and is one call instead of 16 or 128;
 *   - more objects than SIMDs, UNEQUAL extents (4096 objects of 1-16 extents of 4 KiB-256 KiB, longest
 *     first): the grouped walk.  38 ms against 51 ms for the steps and 55 ms for efes_hash_chain;
 *   - more objects than SIMDs, EQUAL extents (4096 objects x 16 x 64 KiB; 16 384 x 4 x 64 KiB): the
 *     grouped walk as ONE call, at 0.29 and 0.11 of efes_hash_chain's time; the steps through
 *     efes_hash_submit (AUTO) where 16 or 4 calls are no burden: they stay 1.14 and 1.21 times faster
 *     than the grouped walk (FED4's producer SIMDs at 4096; four GROUP4 launches without the per-member
 *     refill at 16 384).  efes_hash_chain itself runs one chain per SIMD at a time there: 3.9 and 10.8
 *     times the steps' time.  A forced EFES_MODE_GROUP4 at 4096 objects takes 1.25 times GROUP16's time;
 *   - an array without EFES_JOB_CHAIN (1024 x 4 MiB): efes_hash_submit; the chain call takes 3 to 4 %
 *     longer than EFES_MODE_DEEP for the same bytes. */
#define EFES_HASH_CHAIN_MAX_JOBS (1u << 20)
size_t efes_hash_chain_scratch(uint32_t njobs);
int efes_hash_chain(efes_ctx* ctx, const efes_job* jobs_device, uint32_t njobs, void* scratch_device,
                    size_t scratch_bytes, void* stream);

/* efes_hash_chain with the walk chosen by the caller.  Everything efes_hash_chain takes, and its whole
 * contract: the job array, the chain and validity rules, the statuses, the final states with their stale
 * bytes x[nx:64], the per-member sums, the argument errors, the scratch (efes_hash_chain_scratch(njobs)),
 * no host read-back, allocation or wait.  For every job array and every accepted mode it writes byte for
 * byte what efes_hash_chain writes; the yardstick stays Go's Write; Write; ....
 *   - EFES_MODE_DEEP: the wave walk, the very launches of efes_hash_chain (one chain per wavefront);
 *   - EFES_MODE_GROUP4 / GROUP8 / GROUP16 / GROUP32: the grouped walk for more chains than SIMDs.  A
 *     wavefront holds 64/G chains at once, G lanes each, and advances those whose current member has at
 *     least G whole blocks left together, as the grouped job kernels advance jobs (410 + ~700/G
 *     instructions per block and chain); heads, tails, Sums and members shorter than G blocks go through
 *     the one-wave path, one at a time.  A slot whose chain ends draws the next chain, so chains of
 *     unequal extent counts and sizes keep the wavefront full;
 *   - every other value, EFES_MODE_AUTO included, returns EFES_ERR_ARG: the chain count lives on the
 *     device and the call reads nothing back.
 * efes_hash_chain_auto_mode (host-only; ctx may be NULL: 256 CUs) gives the mode for a caller that knows
 * how many chains (objects) the array holds: EFES_MODE_DEEP up to one chain per SIMD, else the largest G
 * whose 64/G chains per SIMD still hold every chain at once -- GROUP32 up to 2 per SIMD, GROUP16 up to 4,
 * GROUP8 up to 8 -- and GROUP4 beyond.
 * EFES_ABI_VERSION stays 8; a binding detects the two calls by their symbols. */
int efes_hash_chain_mode(efes_ctx* ctx, const efes_job* jobs_device, uint32_t njobs, void* scratch_device,
                         size_t scratch_bytes, void* stream, int mode);
int efes_hash_chain_auto_mode(const efes_ctx* ctx, uint32_t nchains);

/* Checkpoints: the RESUMABLE state of a chain after every member the caller asks for, what `.info` holds
 * after each PATCH (fileinfo.go:10-58): the marshalled SHA-1 state (sha1_efes.go:25-38: h, all 64 bytes
 * of x, nx, len) and the CRC (crc32_efes.go:18-24).  efes_hash_chain(_mode) leaves a chain's state only
 * after its LAST member; a member's FINALIZE sum is a Sum on a copy, which nothing resumes from. */
typedef struct efes_checkpoint {
    efes_sha1_state sha1;   /* 104 bytes: h, x (all 64 bytes, stale ones included), _pad, nx, len */
    efes_crc32_state crc32; /* 4 */
    uint32_t _pad;          /* 0 */
} efes_checkpoint;          /* 112 bytes, 8-byte aligned */
#define EFES_CHECKPOINT_TEXT_BYTES 208 /* 200 (sha1_efes.go:25-38) + 8 (crc32_efes.go:18-24), no NUL */

/* efes_hash_chain_mode that also leaves checkpoints.  It takes over that call's whole contract -- the
 * job array, the chain and validity rules, the statuses, the final states, the per-member sums, the
 * scratch (efes_hash_chain_scratch(njobs)), njobs <= EFES_HASH_CHAIN_MAX_JOBS, no host read-back,
 * allocation or wait -- and everything efes_hash_chain_mode(mode) writes it writes byte for byte the same.
 * mode is EFES_MODE_DEEP (wave walk) or EFES_MODE_GROUP4/8/16/32 (grouped walk); every other value,
 * EFES_MODE_AUTO included, returns EFES_ERR_ARG.
 * ckpt_device: a device array of njobs device pointers, parallel to jobs_device (as dst_device of
 * efes_crc32_copy); ckpt[j] == NULL asks for no checkpoint of member j.  A NULL ckpt_device with
 * njobs > 0 returns EFES_ERR_ARG; njobs == 0 returns EFES_OK and launches nothing; the other argument
 * errors are those of efes_hash_chain_mode.
 *   - member j gets its checkpoint when its Write took effect -- status EFES_OK, or EFES_ERR_STATE raised
 *     at its Sum (sha1.go:107-109), where the state is written -- and it does not carry
 *     EFES_JOB_SUM_ONLY.  Then all 112 bytes of *ckpt[j] are written: sha1 = the chain's SHA-1 state after
 *     THAT member's Write, exactly what *job.sha1 would hold had the call ended there (h, all 64 bytes of
 *     x with their stale bytes, nx, len; _pad 0), all zero bytes for a chain with sha1 == NULL;
 *     crc32.crc = the CRC after that member's Write, 0 for a chain with crc32 == NULL; _pad = 0.  The
 *     yardstick is that of the chain calls: j + 1 successive efes_hash_submit_mode(EFES_MODE_DEEP) calls of
 *     one job each, the states read back after the last;
 *   - nothing is written to *ckpt[j] for a member with status EFES_ERR_ARG, for a member whose Write
 *     panics in Go (nx > 64: EFES_ERR_STATE from the Write) and for an EFES_JOB_SUM_ONLY job.  No byte
 *     outside the 112 bytes of a due checkpoint is ever written through ckpt;
 *   - the caller's contract, not checked: the records are 8-byte aligned and overlap neither each other
 *     nor the states, sums, statuses, job array, pointer array, scratch or data; they are visible to
 *     later work in stream order;
 *   - resuming: a later call (any of the job or chain calls) whose head job does not carry EFES_JOB_INIT
 *     and names states that are copies of ckpt[j].sha1 / ckpt[j].crc32 goes on as the uncut Writes do.
 * The records are stored by kernels of their own (the two walks with one more step where a member ends:
 * the state the walk has stored is read back behind the walk's own fence; DESIGN.md §4 "Chained SHA-1 +
 * CRC, checkpoints"); efes_hash_chain and efes_hash_chain_mode launch what they launched before.
 * EFES_ABI_VERSION stays 8; a binding detects the calls by their symbols.
 * Which path when (measured, profiles/hash_chain_ckpt/bench.json, a record on EVERY extent, the mode that
 * efes_hash_chain_auto_mode gives; DESIGN.md §4 "Chained SHA-1 + CRC, checkpoints" has the table; "steps +
 * copies" = what gave these records before: one efes_hash_submit (AUTO) per extent step and one device copy
 * of all states after each step):
 *   - against efes_hash_chain_mode, the same call without the records (three runs of the
 *     tool): within 0.6 % of its time, either way, on the two 1024-object shapes (DEEP) and on the
 *     ragged 4096-object set (GROUP16), which is what that call's own repetitions differ by; 1.03 to 1.05
 *     at 4096 objects x 16 x 64 KiB and at 4096 x 64 x 4 KiB (GROUP16), which is at or beyond the upper end
 *     of that call's own spread there (its slowest repetition lies 2 to 5 % above its median): the
 *     per-member fence, load and store show when members are short;
 *   - objects of UNEQUAL extent counts or sizes: the checkpoint call, at 0.61 (1024 objects of 1-64 extents
 *     of 4 KiB-1 MiB) and 0.74 to 0.75 (4096 objects of 1-16 extents of 4 KiB-256 KiB) of the steps + copies;
 *   - objects of EQUAL extents: the steps + copies stay faster on the device where their 16 or 64 calls and
 *     copies are no burden -- the checkpoint call takes 1.03 to 1.04 (1024 x 16 x 256 KiB), 1.14 to 1.15
 *     (4096 x 16 x 64 KiB) and 1.41 to 1.42 times (4096 x 64 x 4 KiB) their time, as the chain calls
 *     themselves do against the bare steps -- and the checkpoint call is ONE call;
 *   - the text launch takes 7 to 44 us for 16 384 to 262 144 records, under 1 % of the call that made them.
 *
 * efes_checkpoints_marshal_text: the `.info` texts of n contiguous records, on the device.  Record i
 * gives, at text_device + 208 i, the 200 lower-case hex characters efes_sha1_state_marshal_text gives for
 * ckpt[i].sha1 and then the 8 that efes_crc32_state_marshal_text gives for ckpt[i].crc32; no NUL, nothing
 * behind n * 208 characters is written.  Asynchronous on `stream`; n <= EFES_HASH_CHAIN_MAX_JOBS.
 * EFES_ERR_ARG for a NULL ctx, a larger n, or a NULL pointer with n > 0; n == 0 returns EFES_OK and
 * launches nothing.  The per-object states of an object table go from and to such texts on the device through
 * efes_infos_unmarshal_text and efes_infos_marshal_text ("Object infos", below). */
int efes_hash_chain_checkpoints(efes_ctx* ctx, const efes_job* jobs_device, uint32_t njobs,
                                efes_checkpoint* const* ckpt_device, void* scratch_device, size_t scratch_bytes,
                                void* stream, int mode);
int efes_checkpoints_marshal_text(efes_ctx* ctx, const efes_checkpoint* ckpt_device, uint32_t n, char* text_device,
                                  void* stream);

/* efes_hash_chain by the WIDE walk: one chain per LANE, for very many chains of short members (tens of
 * thousands to a million objects of a few PATCH-sized extents).  It takes over the whole contract of
 * efes_hash_chain -- the job array, EFES_JOB_CHAIN / INIT / FINALIZE / SUM_ONLY and every validity rule, a
 * status for every member (EFES_ERR_STATE exactly where the job kernels raise it), the final states with
 * their stale bytes x[nx:64] (_pad left alone), a 24-byte sum for every FINALIZE member, members of length
 * zero, chains with sha1 or crc32 NULL, njobs <= EFES_HASH_CHAIN_MAX_JOBS, the argument errors, the scratch
 * (efes_hash_chain_scratch(njobs), so one buffer serves every chain call of a stream), no host read-back,
 * allocation or wait -- and writes byte for byte what efes_hash_chain writes for every job array.
 * ckpt_device: NULL for no checkpoints (unlike efes_hash_chain_checkpoints, which refuses NULL: this is one
 * call for both uses); else a device array of njobs record pointers under the contract of
 * efes_hash_chain_checkpoints -- all 112 bytes when the member's Write took effect and it is not
 * EFES_JOB_SUM_ONLY, zeros for a hash the chain does not keep and for _pad, nothing for EFES_ERR_ARG, for a
 * panicking Write or for ckpt[j] == NULL, no byte outside a due record -- and the records are byte for byte
 * those of efes_hash_chain_checkpoints(EFES_MODE_DEEP).
 * After the two prep launches of the chain calls a persistent launch of the WIDE job kernel's workgroup
 * runs: a wavefront draws 64 consecutive chains, lane l walks chain t + l, and the wavefront goes through
 * the members in rounds (round r = every lane's r-th member) as the WIDE job kernel goes through jobs.  The
 * state stays in registers and LDS between members and is stored once per chain.  A wavefront lasts as
 * long as the sum over rounds of its longest member, so arrays sorted longest first suit it, and so do
 * chains of equal extent counts (DESIGN.md §4 "Chained SHA-1 + CRC, wide walk").
 * efes_hash_chain_mode and efes_hash_chain_checkpoints keep refusing EFES_MODE_WIDE, and
 * efes_hash_chain_auto_mode keeps its values.  efes_hash_chain_auto_mode_wide (host-only; ctx may be NULL:
 * 256 CUs) is for a caller that has both: EFES_MODE_WIDE from the measured chain count upwards -- that
 * result goes to efes_hash_chain_wide -- and efes_hash_chain_auto_mode's value below it, which goes to
 * efes_hash_chain_mode.
 * EFES_ABI_VERSION stays 8; a binding detects the two calls by their symbols.
 * Which path when, continued (measured, profiles/hash_chain_wide/bench.json; DESIGN.md §4 "Chained SHA-1 +
 * CRC, wide walk" has the table; fused jobs, medians of device time; "grouped walk" = efes_hash_chain_mode at
 * efes_hash_chain_auto_mode's mode, "steps" as above):
 *   - 32 768 objects and more, EQUAL extents (32 768 x 4 x 32 KiB, 65 536 x 4 x 16 KiB, 262 144 x 4 x 4 KiB):
 *     the wide walk, at 0.43, 0.15 and 0.05 of the grouped walk's time (3.1, 1.6 and 1.7 ms for 4 GiB against
 *     7.3, 10.7 and 32.0).  It equals the steps at 32 768 objects (1.00) and at 65 536 (0.97, inside both
 *     spreads), and takes 0.79 of their time at 262 144; it is ONE call;
 *   - 65 536 objects of UNEQUAL extents (1-8 extents of 4-64 KiB, longest first): the wide walk at 0.74 of
 *     the grouped walk's time (15.4 ms against 20.9 for 9.5 GiB); the steps take 14.6 ms (the wide walk 1.06
 *     times that, outside both spreads): a wavefront lasts as long as the sum over rounds of its longest
 *     member;
 *   - 16 384 objects x 4 x 64 KiB: the grouped walk; the wide walk takes 1.06 times its median (6.1 ms
 *     against 5.8, minimum 5.4) with a quarter of the SIMDs holding a wavefront, the steps 4.6 ms;
 *   - 4096 objects x 64 x 4 KiB: the wide walk takes 0.78 of the grouped walk's time (6.3 ms against 8.1)
 *     although only 64 wavefronts have chains -- the grouped walk sends every short member through the
 *     one-wave path -- and 1.14 times the steps' (5.5 ms).  efes_hash_chain_auto_mode_wide does not pick it
 *     there: at 16 384 objects the wide walk loses, so below 32 768 the count alone does not decide;
 *   - with a record on EVERY extent the wide walk takes 0.98 to 1.02 of its own time without (inside its
 *     spread except at 4096 x 64 x 4 KiB: 1.015 with 262 144 records), so against efes_hash_chain_checkpoints and the steps + copies the ratios are
 *     those above: 0.41, 0.15, 0.06, 0.73 and 0.75 of the checkpoint call on the five shapes it wins, 1.00 at
 *     16 384 objects.
 * efes_hash_chain_auto_mode_wide therefore returns EFES_MODE_WIDE from 32 chains per SIMD (32 768 on 256
 * CUs), the smallest measured count from which the wide walk's median stays below the grouped walk's
 * minimum. */
int efes_hash_chain_wide(efes_ctx* ctx, const efes_job* jobs_device, uint32_t njobs,
                         efes_checkpoint* const* ckpt_device, void* scratch_device, size_t scratch_bytes,
                         void* stream);
int efes_hash_chain_auto_mode_wide(const efes_ctx* ctx, uint32_t nchains);

/* efes_hash_chain_wide that also GATHERS: every byte is written out and hashed by both digests in one pass
 * -- io.MultiWriter(f, CRC32, Sha1) with a device destination as the first writer (filereceiver.go:208-209)
 * -- for an upload whose PATCH-sized extents lie scattered over a staging pool and which is wanted
 * contiguous for the write-out AND with its `.info` digests.
 * The call is efes_hash_chain_wide plus a copy of each member's bytes.  It takes over that call's whole
 * contract: the job array, EFES_JOB_CHAIN / INIT / FINALIZE / SUM_ONLY and every validity rule, a status for
 * every member, the final states with their stale bytes, the per-member sums, ckpt_device with its
 * NULL-means-no-records rule, the scratch (efes_hash_chain_scratch(njobs)), njobs <=
 * EFES_HASH_CHAIN_MAX_JOBS, njobs == 0 returns EFES_OK and launches nothing, the argument errors, no host
 * read-back, allocation or wait.  Everything efes_hash_chain_wide writes for a job array this call writes
 * byte for byte the same.  The copy:
 *   - dst_device is a device array of njobs device pointers, parallel to jobs_device.  dst[j] may have any
 *     alignment, independent of the alignment of jobs[j].data; dst[j] == NULL: member j is hashed and not
 *     copied.  A NULL dst_device with njobs > 0 returns EFES_ERR_ARG: use efes_hash_chain_wide;
 *   - member j is copied when its Write took effect: status EFES_OK, or EFES_ERR_STATE raised at its Sum
 *     (sha1.go:107-109, where the state is written too).  Then exactly [dst[j], dst[j] + length) holds the
 *     source bytes.  A zero-length member writes nothing, and so does every EFES_JOB_SUM_ONLY job;
 *   - nothing is written through dst[j] for a member with status EFES_ERR_ARG, for a member whose Write
 *     panics in Go (nx > 64: EFES_ERR_STATE from the Write) and the members behind it, and for a job that
 *     names neither state, which hashes nothing and copies nothing.  This is tighter than efes_crc32_copy,
 *     which learns validity only after its scan: the wide walk knows it, lane by lane, before it touches
 *     the member's bytes;
 *   - no byte outside a due range is ever written and no destination byte is ever read: the ranges of a
 *     gathered object abut at byte granularity and belong to other lanes and wavefronts, so partial pieces
 *     are narrower stores, never read-modify-write;
 *   - the caller's contract, not checked: destination ranges overlap neither each other nor any source
 *     range, the states, sums, statuses, records, job array, pointer arrays or scratch;
 *   - the destination bytes are visible to later work in stream order, like the states.
 * The walk's kernels with three stores added (kernels of their own; efes_hash_chain_wide launches what it
 * launched before): the bytes that complete a pending x[:nx] and the bytes behind the last whole block go
 * out one by one, every whole block as four 16-byte stores from the registers it is hashed from, at
 * whatever alignment the destination has (DESIGN.md §4 "Chained SHA-1 + CRC, wide walk with copy").
 * EFES_ABI_VERSION stays 8; a binding detects the call by its symbol.
 * Which path when, continued (measured, profiles/hash_chain_wide_copy/bench.json; DESIGN.md §4 "Chained
 * SHA-1 + CRC, wide walk with copy" has the table; fused jobs, every object gathered contiguously, medians
 * of device time; "two calls" = efes_hash_chain_wide, then the best single-launch copy of the same extents):
 *   - 32 768 x 4 x 32 KiB, 65 536 x 4 x 16 KiB and the ragged 65 536 objects of 1-8 extents of 4-64 KiB:
 *     efes_hash_chain_wide_copy, at 0.95, 0.85 and 0.87 of the two calls' time (4.5, 2.7 and 18.1 ms against 4.7,
 *     3.2 and 20.9), its median below the two calls' minimum on all three.  The copy does NOT ride along free,
 *     as it does for efes_crc32_copy: the call takes 1.43, 1.66 and 1.14 times efes_hash_chain_wide alone (3.1,
 *     1.6 and 15.9 ms) and 2.8, 1.7 and 3.6 times the copy alone (1.6, 1.6 and 5.0 ms) -- a lane stores its
 *     block as four 16-byte pieces into a line no other lane of the wavefront touches;
 *   - 262 144 x 4 x 4 KiB: the TWO CALLS.  The fused call takes 1.09 times their time (3.3 ms against 3.0,
 *     minimum 3.0) and twice efes_hash_chain_wide alone (1.7 ms); its median is not below their minimum;
 *   - a record on every extent costs the fused call 1 % or less (0.99 to 1.01 of its time) except at 65 536 x
 *     4 x 16 KiB, where it costs 10 %;
 *   - relative misalignment is not free here: destinations displaced by 1 byte cost 1.32, 1.34, 1.26 and 1.14
 *     times the aligned call on the four shapes, by 8 bytes 1.01, 1.30, 1.23 and 1.03 times.  A caller that
 *     can choose keeps the objects' destinations 16-byte aligned (COPY_ALIGN does);
 *   - efes_hash_chain_wide itself has not moved: its kernels are byte for byte the parent's, and its medians
 *     lie within the spread of the parent's tree on the same machine on every shape;
 *   - below the wide walk's range (fewer than 32 768 objects, or long extents) no fused walk is offered,
 *     and none is needed.  Not measured, but from the rates above: the wave walk and the grouped walk hash
 *     4 GiB in 5.8 to 32 ms, many times the 1.6 ms a copy of 4 GiB takes, so there the hash is many times
 *     slower than the copy and a copy beside it costs a few per cent.  There the caller runs
 *     efes_hash_chain(_mode) and a copy of its own. */
int efes_hash_chain_wide_copy(efes_ctx* ctx, const efes_job* jobs_device, void* const* dst_device,
                              efes_checkpoint* const* ckpt_device, uint32_t njobs, void* scratch_device,
                              size_t scratch_bytes, void* stream);

/* Object tables: the arrays the chain calls take, built ON THE DEVICE.  Every chain call above takes a device
 * array of 56-byte jobs, one per extent; the gather calls add dst[], the checkpoint calls ckpt[].  A job is
 * six pointers and a flag word, and all of them follow from the extent's (offset, length), the object it
 * belongs to and its index, given seven base addresses.  efes_objects_jobs expands an OBJECT TABLE -- the
 * extents and the object boundaries, 16 bytes per extent and 4 per object, in device memory -- into the job
 * array, the destination pointers and the record pointers, in stream order, directly in front of any chain
 * call: a caller whose extents live in a device-side pool needs no round trip through the host, and a host
 * caller uploads 16 instead of up to 72 bytes per extent.  The gather layout falls out of the same scans.
 *
 * efes_objects and efes_objects_out are HOST structs; the pointers in them are device addresses.  Object i
 * owns the extents [first[i], first[i + 1]); an object without extents takes no job.  For extent j let
 * i = owner(j) be the largest i in [0, nobjects) with first[i] <= j (0 if there is none).  Written:
 *   - jobs[j]: data = data + extents[j].offset, length = extents[j].length, sha1 = sha1 ? sha1 + i : NULL,
 *     crc32 = crc32 ? crc32 + i : NULL, sum = sums + 24 j, status = status ? status + j : NULL, _reserved = 0;
 *     flags = EFES_JOB_INIT (EFES_OBJECTS_FRESH) or 0 where j == first[i], EFES_JOB_CHAIN on every other
 *     extent, plus EFES_JOB_FINALIZE where j + 1 == first[i + 1], or on every extent with EFES_OBJECTS_RUNNING;
 *   - out->ckpt[j] = in->ckpt + j (112-byte records), when in->ckpt != NULL;
 *   - out->dst[j] = copy_to + L[i] + within(j), when copy_to != NULL: within(j) is the sum of the lengths of
 *     the object's extents before j and L the layout -- copy_offsets[i] where given, else the exclusive prefix
 *     sum, over the objects before i, of their sizes rounded up to copy_align (a power of two <= 2^20; 0 =
 *     EFES_OBJECTS_COPY_ALIGN): the objects back to back in their order, each start aligned;
 *   - out->layout (may be NULL; may be asked for without copy_to): layout[i] = L[i] for i < nobjects, and
 *     layout[nobjects] = the room the layout needs behind copy_to: L[nobjects - 1] + size[nobjects - 1] in the
 *     default layout, max(copy_offsets[i] + size[i]) with explicit offsets, 0 for no objects.
 * All arithmetic is modulo 2^64.  Nothing outside the named output arrays (and the scratch) is written.
 * SAFETY PROPERTY: every pointer emitted is formed from an index inside [0, nobjects) or [0, nextents),
 * whatever first[] holds.  The fill runs one thread per output element and clamps the owner: the binary
 * search reads first[0, nobjects) only and returns an index of that range, a boundary is read at
 * first[0, nobjects] only and clamped to [0, nextents] before it indexes the scanned lengths.  A table that
 * is not non-decreasing, or whose first[0] != 0 or first[nobjects] != nextents, therefore gives unspecified
 * but in-range jobs (with nobjects == 0 and nextents > 0 the one index there is, 0, is used: such a table
 * has no state to point at and its jobs must not be run).
 * Errors, checked first and without the device: EFES_ERR_ARG for a NULL ctx, in or out and for nobjects or
 * nextents > EFES_OBJECTS_MAX; with nextents > 0 also for NULL extents, first, sums or out->jobs, for sha1 and
 * crc32 both NULL, copy_to without out->dst, in->ckpt without out->ckpt, copy_offsets without copy_to, unknown
 * flag bits, a copy_align that is no power of two or exceeds 2^20, and a scratch that is NULL, not 16-byte
 * aligned or smaller than efes_objects_jobs_scratch(nobjects, nextents) (0 for counts the call refuses).
 * nextents == 0 launches nothing for jobs and needs no scratch; it still writes layout when asked (with
 * nobjects == 0 the single word layout[0] = 0).
 * Asynchronous on `stream` (NULL = the context stream), no host read-back, allocation or wait; the scratch is
 * used in stream order, as the chain calls use theirs.  The outputs are visible to later work in stream
 * order: a chain call queued behind it on the same stream needs no host synchronisation in between.
 * Two-level 64-bit scans of the lengths and of the rounded sizes, a 64-bit maximum by vector atomics, and
 * one fill pass that looks the owner up once per extent and stores every output as contiguous 64-bit words
 * (DESIGN.md §4 "Object tables"); every grid is sized from an element count, none from the CU count.
 *
 * efes_objects_jobs_host is the same function with extents, first, copy_offsets and all of out in HOST
 * memory, and no context, scratch or stream: the base addresses are only added to, never dereferenced.  For
 * a caller whose table is on the host but who does not want to restate the flag rules (the Go binding), and
 * for checking the contract on a machine without a GPU.  The same argument errors, EFES_ERR_NOMEM if its own
 * working arrays cannot be had.
 * EFES_ABI_VERSION stays 8; a binding detects the calls by their symbols.
 * Which path when (measured, profiles/objects_jobs/bench.json; DESIGN.md §4 "Object tables" has the table; fused sets
 * with a record per extent and the default gather layout, so all three arrays are made; "host build" = the numpy
 * fill of the three arrays from packed extent and count arrays, their upload and a synchronise, "device build" =
 * the upload of the table, this call and a synchronise, both wall-clock medians):
 *   - on every shape measured: the device build, at 0.03 to 0.08 of the host build's time, its median below the
 *     host build's minimum on all five -- 0.16 ms against 1.9 (32 768 objects x 4 extents), 0.32 against 4.2
 *     (65 536 x 4), 0.24 against 3.8 (4096 x 64), 0.33 against 5.4 (65 536 objects of 1-8 extents) and 0.86 ms
 *     against 31.6 (262 144 x 4, 1 048 576 extents);
 *   - the call alone takes 25, 29, 29, 33 and 55 us of device time on these shapes: 0.8, 1.8, 0.4, 0.2 and 3.9 % of
 *     the efes_hash_chain_wide call behind it (3.1, 1.6, 6.6, 15.9 and 1.4 ms).  The host build takes 0.3 to 2.6
 *     times that walk's time, and 22 times at 262 144 x 4: 31.6 ms of host work in front of a 1.4 ms walk;
 *   - the call is NOT bandwidth-bound at these sizes, as it was expected to be: 0.5 to 1.7 TB/s read plus written,
 *     6 to 22 % of the 8 TB/s HBM peak.  Its five or six launches of a few microseconds each are what it costs;
 *   - neither build is what a Python caller pays for first: flattening Python lists of extents into the packed
 *     arrays takes 34 to 460 ms on these shapes, more than either build.  A caller with many objects keeps its
 *     extents packed, or on the device (DeviceObjects.from_table). */
typedef struct efes_extent {
    uint64_t offset; /* extent j lies at data + offset */
    uint64_t length;
} efes_extent; /* 16 bytes */

#define EFES_OBJECTS_FRESH 0x1u   /* every object's first extent carries EFES_JOB_INIT */
#define EFES_OBJECTS_RUNNING 0x2u /* every extent carries EFES_JOB_FINALIZE; else each object's last one */
#define EFES_OBJECTS_MAX EFES_HASH_CHAIN_MAX_JOBS /* nobjects and nextents, each */
#define EFES_OBJECTS_COPY_ALIGN 256u

typedef struct efes_objects {      /* a HOST struct; the pointers in it are device addresses */
    const void* data;              /* extent j lies at data + extents[j].offset */
    const efes_extent* extents;    /* nextents */
    const uint32_t* first;         /* nobjects + 1: object i owns extents [first[i], first[i+1]) */
    efes_sha1_state* sha1;         /* nobjects states, or NULL: no SHA-1 */
    efes_crc32_state* crc32;       /* nobjects states, or NULL: no CRC */
    uint8_t* sums;                 /* 24 * nextents */
    int32_t* status;               /* nextents, or NULL */
    efes_checkpoint* ckpt;         /* nextents records, or NULL: no record pointers */
    void* copy_to;                 /* or NULL: no destination pointers */
    const uint64_t* copy_offsets;  /* nobjects, or NULL: the default layout */
    uint32_t nobjects, nextents, flags, copy_align; /* copy_align 0 = EFES_OBJECTS_COPY_ALIGN */
} efes_objects; /* 96 bytes: ten pointers, four 32-bit words */

typedef struct efes_objects_out { /* a HOST struct of device addresses */
    efes_job* jobs;               /* nextents */
    void** dst;                   /* nextents; needed exactly when copy_to != NULL */
    efes_checkpoint** ckpt;       /* nextents; needed exactly when in->ckpt != NULL */
    uint64_t* layout;             /* nobjects + 1, or NULL */
} efes_objects_out; /* 32 bytes */

size_t efes_objects_jobs_scratch(uint32_t nobjects, uint32_t nextents);
int efes_objects_jobs(efes_ctx* ctx, const efes_objects* in, const efes_objects_out* out, void* scratch_device,
                      size_t scratch_bytes, void* stream);
int efes_objects_jobs_host(const efes_objects* in, const efes_objects_out* out);

/* Object results: what a chain call left for an object table, sorted out ON THE DEVICE.  The walks leave a
 * 24-byte sum and a status per EXTENT; every caller asks per OBJECT, and what it asks is a check: the objects
 * re-checked after a copy or drain, the gather before a write-out, the uploader that compares its SHA-1 with the
 * efes-file-sha1 the server returned and fails on a mismatch (write.go:112-114).  efes_objects_results takes the
 * table efes_objects_jobs was given and the sums and statuses behind it, and writes one 32-byte result per object
 * (digest, status, verdict against an expected digest), the ascending list of the objects that are not in order,
 * and four counters: a caller that only wants to know whether everything matched reads back 16 bytes.
 *
 * `in` is the very table efes_objects_jobs was given; only first, sums, status, nobjects and nextents of it are
 * read, never the extents or the data.  Object i owns the extents [first[i], first[i + 1]):
 *   - an object with no extents gets 24 zero bytes, status EFES_OK and verdict EFES_VERDICT_EMPTY; its expected
 *     entry is never read;
 *   - otherwise let l = first[i + 1] - 1.  status is the status of the lowest-indexed member whose status is not
 *     EFES_OK, else EFES_OK.  sum is sums[24 l, 24 l + 24) when status[l] == EFES_OK, otherwise 24 zero bytes: a
 *     member that failed wrote no sum, so stale bytes are never reported;
 *   - verdict: FAILED when the object's status is not EFES_OK (expected is not read for it); otherwise MISMATCH
 *     when expected != NULL and a byte range selected by `compare` differs (EFES_HASH_SHA1: bytes 0..19,
 *     EFES_HASH_CRC32: bytes 20..23; compare == 0 compares nothing); otherwise OK;
 *   - bad[k] is the index of the k-th object, in ascending order, whose verdict is MISMATCH or FAILED: exactly
 *     counts[1] + counts[2] words are written and nothing behind them; the list is sorted, not "some order";
 *   - counts[v] = the objects with verdict v; always written, all four words, all zeros for nobjects == 0.
 * Nothing outside the named outputs (and the scratch) is written; results and bad may each be NULL.
 * The caller's contract, documented and not checked: the sums and statuses are those a chain call left for
 * `in`'s job array, each object's last extent carried EFES_JOB_FINALIZE (as efes_objects_jobs tables do), and the
 * outputs overlap nothing else.
 * SAFETY PROPERTY, as for efes_objects_jobs: every index that forms an address is clamped into [0, nobjects) or
 * [0, nextents), whatever first[] holds (the same owner search and boundary clamp).  A table that is not
 * non-decreasing gives unspecified but in-range results.
 * Errors, checked first and without the device: EFES_ERR_ARG for a NULL ctx, in or req, a NULL counts, nobjects or
 * nextents > EFES_OBJECTS_MAX, unknown compare bits or a nonzero _reserved; with nobjects > 0 a NULL first; with
 * nextents > 0 a NULL sums or status (a table built without a status array is refused); sums or expected not
 * 4-byte aligned; results not 8-byte aligned, bad or counts not 4-byte aligned; and, with nobjects > 0, a scratch
 * that is NULL, not 16-byte aligned or smaller than efes_objects_results_scratch(nobjects, nextents) (0 for counts
 * the call refuses, never 0 otherwise).  nobjects == 0 needs no scratch.  A refused call writes nothing.
 * Asynchronous on `stream` (NULL = the context stream), no host read-back, allocation or wait: queued behind a
 * chain call on the same stream it needs no synchronisation in between.
 * No lane loops over an object's members (one object may own all 2^20 extents): the first failing member is found
 * with one lane per extent -- the owner by the builder's binary search, only for a member that failed, then a
 * 32-bit atomic minimum of the member's index into a per-object word of the scratch, which the call sets to
 * "none" itself, in stream order; the per-object pass reads that word, the status it names, the last member's
 * status where that is another one, and at most one sum, and compares it as six 32-bit words under the two
 * masks; the bad list is a two-level exclusive scan of the bad flags, each lane storing its own index at its
 * rank; the counters are the sums of per-workgroup counts, so counts[1] + counts[2] is the scan's total.  Every
 * grid is sized from an element count (DESIGN.md §4 "Object results").
 *
 * efes_objects_results_host is the same function with every array in HOST memory and no context, scratch or
 * stream: for a caller that already has the sums on the host, and for checking the rules on a machine without a
 * GPU.  The same argument errors, EFES_ERR_NOMEM if its own working array cannot be had.
 * EFES_ABI_VERSION stays 8; a binding detects the calls by their symbols.
 * Which path when (measured, profiles/objects_results/bench.json; DESIGN.md §4 "Object results" has the table; sets
 * of the builder's five shapes with random sums, every status EFES_OK and none or 1 % of the expected digests spoiled;
 * "verify" = DeviceObjects.verify(): this call with `expected` on the device, a synchronise, the 16 bytes of counts
 * and then the bad list to the host; "host path" = what the library offered before: the 24 + 4 bytes per extent
 * copied to the host and a VECTORISED numpy pick of the last extents and compare; wall-clock, verify's median
 * against the host path's minimum):
 *   - on the builder's five shapes: this call, in every case measured.  With no bad object verify takes 0.049 ms
 *     against 0.95 (32 768 objects x 4 extents), 0.051 against 1.76 (65 536 x 4), 0.048 against 0.43 (4096 x 64), 0.047
 *     against 2.31 (65 536 objects of 1-8 extents) and 0.23 ms against 7.66 (262 144 x 4, 1 048 576 extents): 0.02 to
 *     0.11 of the host path's time; with 1 % of the digests differing 0.063, 0.071, 0.063, 0.062 and 0.22 ms against
 *     0.89, 1.82, 0.43, 2.29 and 7.42: 0.03 to 0.15.  With `expected` uploaded from host memory in front of the call
 *     (24 bytes per object) it is 0.03 to 0.16.  One table outside those shapes has the host path ahead: see below;
 *   - the host path is nearest at 4096 x 64, where it picks only 4096 sums out of the 7 MB it copies;
 *   - the call alone takes 15 to 19 us of device time (a memset and three kernels), the 32-byte records 0.1 to 1.2 us
 *     more: launches, not bytes.  What verify takes beyond it is the synchronise and two small copies;
 *   - a caller that wants every digest on the host anyway (sha1_hex() of every object) still copies them: results()
 *     brings 32 bytes per object instead of 28 per extent, which was not timed here;
 *   - all of the figures above are for tables WITHOUT failed members, where the per-extent pass takes no owner search
 *     and no atomic minimum.  With a failed member in 1 % of the objects the call takes 17 to 26 us and verify stays at
 *     0.02 to 0.15 of the host path; with EVERY member failed (4 to 64 atomic minima on each word) the call takes 26
 *     to 67 us and verify 0.05 to 0.19 of the host path (0.40 ms against 7.9 at 262 144 x 4);
 *   - the HOST PATH IS AHEAD in one case: ONE object that owns all 1 048 576 extents with EVERY member failed.  All
 *     1 048 576 atomic minima then fall on one word and the call takes 11.9 ms, against 1.0 ms for the host path;
 *     the same table with no failed member takes 15 us (verify 0.051 ms against 0.95).  Such a table is a chain
 *     that broke at its first member; a reduction over the wavefront in front of the atomic would take the count
 *     to one per wavefront and is not built.  A caller that expects most members of very long objects to have
 *     failed reads the statuses back instead. */
#define EFES_VERDICT_OK       0u /* every member EFES_OK, and every digest that was compared is equal */
#define EFES_VERDICT_MISMATCH 1u /* every member EFES_OK, a compared digest differs */
#define EFES_VERDICT_FAILED   2u /* some member's status is not EFES_OK */
#define EFES_VERDICT_EMPTY    3u /* the object owns no extents: no job ran, nothing to compare */

typedef struct efes_object_result {
    uint8_t  sum[24];  /* the 24-byte sum of the object's LAST extent (SHA-1 Sum, then CRC big-endian) */
    int32_t  status;   /* the status of the object's FIRST member that is not EFES_OK, else EFES_OK */
    uint32_t verdict;  /* EFES_VERDICT_* */
} efes_object_result;  /* 32 bytes */

typedef struct efes_results {       /* a HOST struct of device addresses */
    const uint8_t* expected;        /* 24 * nobjects, laid out like a sum, or NULL: nothing is compared */
    uint32_t compare;               /* EFES_HASH_SHA1 (bytes 0..19) | EFES_HASH_CRC32 (bytes 20..23); 0 allowed */
    uint32_t _reserved;             /* 0 */
    efes_object_result* results;    /* nobjects, or NULL */
    uint32_t* bad;                  /* nobjects words, or NULL: the objects with verdict MISMATCH or FAILED, ascending */
    uint32_t* counts;               /* 4 words, required: counts[v] = objects with verdict v */
} efes_results; /* 40 bytes */

size_t efes_objects_results_scratch(uint32_t nobjects, uint32_t nextents);
int efes_objects_results(efes_ctx* ctx, const efes_objects* in, const efes_results* req, void* scratch_device,
                         size_t scratch_bytes, void* stream);
int efes_objects_results_host(const efes_objects* in, const efes_results* req);

/* Object order: the LONGEST-FIRST order of an object table's chains, made ON THE DEVICE.  Every walk depends on
 * the order of the chains in its job array: the wide walk gives 64 consecutive chains to one wavefront, which
 * lasts as long as its longest member in every round, and the wave and grouped walks draw whole chains from the
 * array in order, so long chains at the end leave the launch on a few busy SIMDs.  efes_plan_batch orders host
 * jobs by host lengths; for an object table efes_objects_order ranks the objects by size and
 * efes_objects_jobs_ordered emits the job array in that (or any) order, both in stream order in front of the walk.
 * The builder's records address the states by object index and the sums, statuses and records by table extent
 * index, so only the job array and its two parallel pointer arrays are permuted: everything the walks write stays
 * in TABLE order, and efes_objects_results and the gather layout work on an ordered set unchanged.
 *
 * efes_objects_order writes order[0, nobjects): order[r] is the table index of the object at rank r.  The key of
 * object i is its byte size as the builder computes it, E[bound(first, i + 1)] - E[bound(first, i)] modulo 2^64,
 * E the running sum of the lengths and bound() the clamp of first[] to [0, nextents].  Descending size; equal
 * sizes in ascending table index: a total order, so the result is one fixed permutation and the device call and
 * the host twin give the same words.  Only extents[].length, first, nobjects and nextents of `in` are read, never
 * the data or the other base addresses.
 * SAFETY PROPERTY: whatever first[] holds, order is a permutation of [0, nobjects).
 * Errors, checked first and without the device: EFES_ERR_ARG for a NULL ctx or in, nobjects or nextents >
 * EFES_OBJECTS_MAX; with nextents > 0 a NULL extents; with nobjects > 0 a NULL first, a NULL or not 4-byte aligned
 * order, and a scratch that is NULL, not 16-byte aligned or smaller than efes_objects_order_scratch(nobjects,
 * nextents) (0 for counts the call refuses, never 0 otherwise).  A refused call writes nothing.  nobjects == 0
 * returns EFES_OK, launches nothing and writes nothing; with nextents == 0 every size is 0 and the order is the
 * identity.
 * Asynchronous on `stream` (NULL = the context stream), no host read-back, allocation or wait; the scratch is used
 * in stream order.
 * A stable LSD radix sort of (key = bitwise NOT of the size, value = object index) pairs, radix 256, from the
 * identity, so stability gives the tie rule.  Each digit pass is three launches -- the digit counts of every tile
 * of 1024 pairs, the two-level scan of those counts, a stable scatter (ranks within a wavefront by ballots, across
 * the tile's wavefronts by a table in LDS) -- and no wave waits for another.  Real sizes fill two or three of the
 * eight key bytes: the pass that makes the keys also ORs key[i] ^ key[0] over all i into one word, and the
 * launches of a digit in which all keys agree return at once; which of the two buffers a pass reads follows on
 * the device from that word.  The number of launches is fixed by the counts (DESIGN.md §4 "Object order").
 *
 * efes_objects_jobs_ordered is efes_objects_jobs that emits the objects in the order given: the output of
 * efes_objects_order or any permutation the caller has (its own priority order).  The whole contract of
 * efes_objects_jobs holds, with the same table and the same argument errors; in addition EFES_ERR_ARG for a NULL
 * order with nobjects > 0 and for an order or job_first that is not 4-byte aligned, and the scratch is measured by
 * efes_objects_jobs_ordered_scratch.  Let cnt(i) = bound(first, i + 1) - bound(first, i), 0 where that is
 * negative, and J[r] the exclusive prefix sum of cnt(order[r]).  Slot k in [J[r], J[r + 1]) belongs to object
 * i = order[r], extent j = bound(first, i) + (k - J[r]):
 *   - jobs[k] is, byte for byte, the record efes_objects_jobs writes at jobs[j]: the same data, length, sha1 + i,
 *     crc32 + i, sums + 24 j, status + j and flag word;
 *   - out->dst[k] and out->ckpt[k] are the values efes_objects_jobs writes at dst[j] and ckpt[j];
 *   - out->layout is unchanged: the gather layout is a property of the table, not of the job order;
 *   - job_first (may be NULL; else nobjects + 1 words): job_first[r] = J[r], saturated at nextents -- the slots a
 *     rank owns.  Without extents it is all zeros.
 * With the identity order and a well-formed table every output is byte for byte that of efes_objects_jobs.
 * SAFETY PROPERTY, as for the builder: order[r] is clamped into [0, nobjects), the rank of a slot is an index of
 * that range, j is clamped into [0, nextents), and every slot k < nextents is written.  An order that is not a
 * permutation, or a malformed first[], gives unspecified but in-range jobs that must not be run.
 * Asynchronous and stream-ordered like the builder: a chain call queued behind it on the same stream needs no
 * host synchronisation.  The scans of the lengths and of the rounded sizes are the builder's; added are a scan of
 * cnt(order[r]) and a fill pass of one lane per output SLOT: a binary search of J for the rank, then the builder's
 * LDS-staged, wavefront-contiguous stores of the seven job words.
 *
 * The two _host twins are the same functions over HOST arrays, with no context, scratch or stream, like
 * efes_objects_jobs_host; EFES_ERR_NOMEM if their working arrays cannot be had.
 * EFES_ABI_VERSION stays 8; a binding detects the calls by their symbols.
 * Which path when (measured, profiles/objects_order/bench.json; DESIGN.md §4 "Object order" has the table; fused sets
 * over a 4 GiB pool whose tables were SHUFFLED by a fixed seed, walked by the call DeviceObjects(walk="auto_wide")
 * picks; device time, medians; "table" = efes_objects_jobs + the walk, "ordered" = efes_objects_order +
 * efes_objects_jobs_ordered + the walk, the project's rule: a median below the other path's minimum):
 *   - the expected gain is NOT there: on none of the four shapes is the longest-first order faster than the shuffled
 *     table's own, and on two it is slower.  The walk alone over longest-first jobs takes 1.12 times its time over the
 *     shuffled jobs on the ragged wide-walk set (65 536 objects of 1-8 extents of 4-64 KiB: 15.98 ms against 14.31),
 *     1.05 times on the ragged grouped-walk set (4096 objects of 1-16 extents of 4-256 KiB, EFES_MODE_GROUP16: 38.06
 *     against 36.20), and the same within the spread on the ragged wave-walk set (1024 objects of 1-64 extents of
 *     4 KiB-1 MiB: 448.9 against 447.9) and on 65 536 x 4 x 16 KiB (2.743 against 2.734).  With the two calls in
 *     front, "ordered" takes 1.04, 1.05, 1.003 and 1.03 times "table"; the table-order median is below the ordered
 *     minimum on the three ragged shapes.  So order="table" stays the default, and a table in upload order or straight
 *     from a pool is best walked as it is;
 *   - the walk over the device-ordered jobs equals the walk over a table sorted on the host beforehand (1.00 on
 *     every shape: the same job order), and that is the figure the ragged rows of the chain sections quote: the 15.9 ms
 *     of the ragged wide-walk row is 1.12 times what the same set takes shuffled.  "Arrays sorted longest first suit
 *     it" (efes_hash_chain_wide) is not what this run shows against a random order; it was never measured against one;
 *   - what the calls cost: efes_objects_order 91, 79, 77 and 77 us of device time on the four shapes (some thirty
 *     launches of a few microseconds, most of which return at once: real sizes fill three key bytes),
 *     efes_objects_jobs_ordered 43, 52, 50 and 57 us (minima 30, 21, 20 and 26): together 0.8 %, 0.3 %, 0.03 % and
 *     4.9 % of the walk behind them.  On the equal shape, where no order can gain, that 4.9 % is the whole effect;
 *   - a caller that WANTS a given order -- longest first for a consumer that drains results in that order, its own
 *     priority order through efes_objects_jobs_ordered -- gets it without the round trip: against copying the table
 *     to the host, a numpy stable sort, permuting and uploading it and efes_objects_jobs, wall-clock from the table
 *     on the device to the synchronise behind the walk, 15.8 ms against 30.4 (minimum 24.1) on the ragged wide-walk
 *     set and 2.84 against 5.24 on 65 536 x 4 x 16 KiB, the median below the host path's minimum; 38.2 against 38.9
 *     on the grouped-walk set, also below its minimum; no difference on the wave-walk set (449.2 against 449.1), whose
 *     walk hides both.  And only this path leaves the sums, statuses and results in TABLE order: the host path
 *     permutes the table, so everything comes back in sorted order. */
size_t efes_objects_order_scratch(uint32_t nobjects, uint32_t nextents);
int efes_objects_order(efes_ctx* ctx, const efes_objects* in, uint32_t* order_device, void* scratch_device,
                       size_t scratch_bytes, void* stream);
int efes_objects_order_host(const efes_objects* in, uint32_t* order);

size_t efes_objects_jobs_ordered_scratch(uint32_t nobjects, uint32_t nextents);
int efes_objects_jobs_ordered(efes_ctx* ctx, const efes_objects* in, const efes_objects_out* out,
                              const uint32_t* order_device, uint32_t* job_first_device, void* scratch_device,
                              size_t scratch_bytes, void* stream);
int efes_objects_jobs_ordered_host(const efes_objects* in, const efes_objects_out* out, const uint32_t* order,
                                   uint32_t* job_first);

/* Object infos: the per-object states of an object table FROM and TO their `.info` texts, ON THE DEVICE.  A PATCH
 * that is not an upload's first resumes both digests from the texts in `<path>.info` (filereceiver.go:182-188,
 * fileinfo.go:29-45, sha1_efes.go:40-64, crc32_efes.go:26-40) and writes the new texts back behind it
 * (filereceiver.go:226, fileinfo.go:47-58).  For an object table those are efes_infos_unmarshal_text in front of
 * efes_objects_jobs and efes_infos_marshal_text behind efes_objects_results: texts -> states -> builder -> walk ->
 * results -> texts is one chain of stream-ordered calls with no host synchronisation in it.
 *
 * efes_infos is a HOST struct; the pointers in it are device addresses (host addresses for the _host twins).
 * Record i is the EFES_INFO_TEXT_BYTES characters at text + 208 i: the 200 of the SHA-1 state's MarshalText
 * (sha1_efes.go:25-38), then the 8 of the CRC's (crc32_efes.go:18-24), no NUL -- the layout of
 * efes_checkpoints_marshal_text.  A length error cannot arise from this layout: a caller whose text for an object
 * has another length (Go: errInvalidDigest) fills that record with a character that is no hex digit.
 *
 * efes_infos_unmarshal_text, per record i.  The text is VALID when all 208 characters are hex digits as Go's
 * encoding/hex accepts them (0-9, a-f, A-F); all 208 are checked even when sha1 or crc32 is NULL, because an `.info`
 * record always holds both.
 *   - valid: sha1[i] holds exactly what efes_sha1_state_unmarshal_text gives for characters 0..199, and _pad is
 *     written as 0; nx is stored as decoded, whatever its value, as Go does on a 64-bit int; crc32[i].crc is the
 *     big-endian decode of characters 200..207; status[i] = EFES_OK;
 *   - invalid: sha1[i] becomes the REFUSING STATE -- every byte 0 except nx = EFES_SHA1_NX_REFUSED --,
 *     crc32[i].crc = 0, status[i] = EFES_ERR_INVALID_DIGEST.  Go fails that one upload (errInvalidDigest -> 500) and
 *     hashes nothing for it; the refusing state does the same for an object of a table, and uses only what the job
 *     and chain kernels already promise for nx > 64 (sha1.go:62): every Write into it gets EFES_ERR_STATE and writes
 *     nothing, the members behind it get the same, nothing is gathered and no record is stored, and
 *     efes_objects_results reports EFES_VERDICT_FAILED.  The other objects of the table run;
 *   - a CRC-ONLY table (sha1 == NULL) has no such state: the CRC of an invalid text is 0, which hashes like any
 *     other start.  Such a caller reads counts[1] or status before it trusts the CRCs;
 *   - every word of every state of [0, n) is written by every call, so nothing stale survives; nothing outside the
 *     named arrays is written;
 *   - counts (may be NULL) is written whole: counts[0] = valid texts, counts[1] = invalid ones, {0, 0} for n == 0.
 * efes_infos_marshal_text, per record i: characters 0..199 are those of efes_sha1_state_marshal_text(&sha1[i]), or
 * 200 x '0' when sha1 == NULL -- what a checkpoint record holds for a chain without SHA-1 --, characters 200..207
 * those of efes_crc32_state_marshal_text(&crc32[i]), or 8 x '0'.  Lower-case hex, no NUL, nothing behind 208 n is
 * written; status and counts are ignored.  A pure codec: a refusing state marshals like any other, and _pad is not
 * read.
 * Both calls are asynchronous on `stream` (NULL = the context stream) and need no scratch, host read-back,
 * allocation or wait; their outputs are visible to later work in stream order, so efes_objects_jobs and a walk queue
 * directly behind an unmarshal.  The caller's contract, not checked: the arrays overlap neither each other nor
 * anything else in use.
 * Errors, checked first and without the device: EFES_ERR_ARG for a NULL ctx (device calls) or in, n >
 * EFES_OBJECTS_MAX, a nonzero _reserved; with n > 0 a NULL text, or sha1 and crc32 both NULL; sha1 not 8-byte
 * aligned; crc32, status or counts not 4-byte aligned; and, on the device calls only, text not 8-byte aligned.  A
 * refused call writes nothing.  n == 0 returns EFES_OK; unmarshal still writes counts when given, and nothing else
 * is launched.
 * 32 lanes per record, one text word of 8 characters (one 64-bit load or store) and one 32-bit state word per lane;
 * the verdict of a record is a ballot masked to its half of the wavefront, and the lanes store either the decoded
 * word or the refusing image's at the same place; counts start at {n, 0} in stream order, and only a workgroup
 * that holds invalid records moves their number over with two vector atomics.  Every grid is sized from n
 * (DESIGN.md §4 "Object infos").
 *
 * The two _host twins are the same functions over HOST arrays, with no context and no stream; they take text at any
 * alignment.  For a caller whose texts or states are on the host anyway, and for checking the rules on a machine
 * without a GPU.
 * EFES_ABI_VERSION stays 8; a binding detects the calls by their symbols.
 * Which path when (measured, profiles/infos/bench.json, tools/bench_infos.py; DESIGN.md §4 "Object infos" has the
 * table; 4096, 32 768, 65 536, 262 144 and 1 048 576 records of random states, 1 % of the texts spoiled; wall-clock,
 * nine repetitions, a path wins where its median is below the other's minimum; "device path" = the texts from host
 * memory to the device, the call, a synchronise; "host path" = the host twin, the states and CRCs to the device
 * (108 bytes per object), a synchronise; for marshal the mirror image, call + 208 n bytes to the host against 108 n
 * bytes to the host + the twin):
 *   - unmarshal, on all five counts: the DEVICE path, at 0.11, 0.047, 0.038, 0.032 and 0.031 of the host path's
 *     time -- 0.064 ms against 0.59, 0.21 against 4.4, 0.33 against 8.8, 1.10 against 35.1 and 4.4 ms against 146.7
 *     -- although it uploads 208 bytes per object where the host path uploads 108: the twin's decode is what the
 *     host path spends;
 *   - marshal, on all five counts: the DEVICE path, at 0.15, 0.048, 0.044, 0.040 and 0.039 of the host path's time
 *     (0.070 ms against 0.46 up to 4.1 ms against 109.8);
 *   - what the library offered before, efes_sha1_state_unmarshal_text and efes_crc32_state_unmarshal_text per object
 *     through the Python binding, then the same upload: 11.2, 90.0 and 184.8 ms at 4096, 32 768 and 65 536 records
 *     (not timed beyond), 175 to 560 times the device path;
 *   - the calls alone, device time: unmarshal 10, 16, 23, 64 and 224 us, marshal 6, 7, 11, 30 and 136 us.  Up to
 *     65 536 records that is launches, as expected; beyond it is bytes: 1.3 to 1.5 TB/s read plus written for
 *     unmarshal, 2.4 to 2.8 for marshal, of the 8 TB/s HBM peak;
 *   - the counters were NOT free as first built (every workgroup adding both sums: profiles/infos/
 *     bench_every_workgroup_adds.json): 131 072 workgroups' atomics on two words made the unmarshal call 1.61 ms at
 *     1 048 576 records and 0.41 ms at 262 144, six to seven times what it takes now.  Now only a workgroup with an invalid
 *     text touches them; with EVERY text invalid the call takes 12, 33, 56, 197 and 760 us. */
#define EFES_INFO_TEXT_BYTES EFES_CHECKPOINT_TEXT_BYTES /* 208: 200 (sha1_efes.go:25-38) + 8 (crc32_efes.go:18-24), no NUL */
#define EFES_SHA1_NX_REFUSED 65                         /* nx of the refusing state: the smallest nx a Write refuses */

typedef struct efes_infos {     /* a HOST struct; the pointers are device addresses (host addresses for the _host twins) */
    char*             text;     /* 208 * n characters; record i at text + 208 i */
    efes_sha1_state*  sha1;     /* n states, or NULL */
    efes_crc32_state* crc32;    /* n states, or NULL */
    int32_t*          status;   /* n words, or NULL; written by unmarshal only */
    uint32_t*         counts;   /* 2 words, or NULL; written by unmarshal only: [0] valid texts, [1] invalid */
    uint32_t n, _reserved;      /* _reserved 0 */
} efes_infos;                   /* 48 bytes */

int efes_infos_unmarshal_text(efes_ctx* ctx, const efes_infos* in, void* stream);
int efes_infos_marshal_text(efes_ctx* ctx, const efes_infos* in, void* stream);
int efes_infos_unmarshal_text_host(const efes_infos* in);
int efes_infos_marshal_text_host(const efes_infos* in);

/* PATCH logs: the object table of an arrival log of PATCH requests, made ON THE DEVICE.  Every call of the object
 * pipeline takes a finished table -- extents[] grouped by object and in byte order, plus first[] -- but a storage
 * server receives PATCH requests in arrival order, interleaved over its uploads, and saveFile (filereceiver.go:171-227)
 * decides what becomes of each before a byte is hashed.  efes_patches_table applies those rules per upload, in arrival
 * order, and writes the table efes_objects_jobs takes as it is, the answer every request gets and the new
 * FileInfo.Offset of every upload: log -> table -> builder -> walk is one chain of stream-ordered calls.
 *
 * efes_patches is a HOST struct; the pointers in it are device addresses (host addresses for the _host twin).
 * The rules, per object i = p.object in arrival order, arithmetic modulo 2^64 (cur starts at offsets[i], or 0):
 *   - p.object >= nobjects: EFES_PATCH_INVALID, answer offset 0; no upload is touched;
 *   - the object is closed (below): EFES_PATCH_DEFERRED, answer offset cur;
 *   - p.file_offset == 0 (filereceiver.go:174-180, a restart with fresh digests): if a PATCH of i was already
 *     admitted in this log the object closes and the PATCH is DEFERRED; otherwise i is RESTARTED, cur = p.length;
 *   - else p.file_offset == cur: cur += p.length;
 *   - else EFES_PATCH_CONFLICT (409, :186-187), answer offset cur, the required offset;
 *   - an admitted PATCH with cur == p.file_length (:219-224) is EFES_PATCH_DONE and closes the object; any other is
 *     EFES_PATCH_ADMITTED (:226).  Both answer with the new cur.
 * DEFERRED is the one verdict that is no Go answer.  One table holds one chain per object, so a restart behind
 * admitted bytes and anything behind a DONE wait: they come back untouched and in order, and resubmitting them in
 * the next log with the offsets updated (0 and fresh states after a DONE, as Go's deleted `.info` gives) yields what
 * Go's sequential handling yields.
 * The table: the slots are the log stably sorted by min(object, nobjects - 1), so an INVALID record lies in the last
 * object's segment; first[i] is the first slot of object i and first[nobjects] == npatches; slot k of an ADMITTED or
 * DONE PATCH holds {data_offset, length}, every other slot {0, 0}.  Zero-length members are legal in every chain
 * call and write nothing, so nextents == npatches is known on the host and no count has to come back before
 * efes_objects_jobs is queued.  answers[a] (arrival order) holds the verdict, the answer's offset and the slot;
 * patch_of[k] the arrival index of slot k; objects[i] = {cur, EFES_PATCH_OBJ_*, admitted PATCHes}; counts[v] the
 * PATCHes with verdict v.  For a RESTARTED object sha1[i] becomes NewSha1() (x, nx, len and _pad zero) and
 * crc32[i].crc 0; no other state is written.  With running sums (EFES_OBJECTS_RUNNING) the digests of a DONE PATCH
 * are at sums + 24 * slot.
 * Safety: every index that forms an address is clamped; whatever the log holds, first[] is non-decreasing from 0 to
 * npatches and patch_of is a permutation; nothing outside the named outputs and the scratch is written.
 * Errors, checked first and without the device: EFES_ERR_ARG for a NULL ctx (device call) or in; nobjects or
 * npatches above EFES_OBJECTS_MAX; npatches > 0 with nobjects == 0; a NULL first, or with npatches > 0 a NULL log or
 * extents; log, offsets, sha1, extents, answers or objects not 8-byte aligned; crc32, first, patch_of or counts not
 * 4-byte aligned; and, on the device call, a scratch that is NULL, not 16-byte aligned or smaller than
 * efes_patches_table_scratch(nobjects, npatches).  A refused call writes nothing.  With npatches == 0 the call
 * writes first (all zeros), objects and counts and launches nothing else.
 * The device call is asynchronous on `stream` (NULL = the context stream): no host read-back, allocation or wait.
 * A stable LSD radix-256 sort of (key, arrival index), one digit pass up to 256 objects, two up to 65 536, three
 * beyond, fixed on the host; first[] by a lower bound per object in the sorted keys; then the admission pass, the
 * one serial dependency: an object of at most 64 PATCHes is walked by one lane, a longer one by a whole wavefront
 * that loads 64 records at a time and resolves them run by run with ballots.  counts start at {npatches, 0, 0, 0, 0}
 * and only a workgroup that holds another verdict than ADMITTED moves its numbers over with vector atomics
 * (DESIGN.md §4 "PATCH logs").
 * The _host twin is the same function over HOST arrays, with no context, stream or scratch.
 * EFES_ABI_VERSION stays 8; a binding detects the calls by their symbols.
 * Which path when (measured, profiles/patches/bench.json, tools/bench_patches.py; DESIGN.md §4 "PATCH logs" has the
 * table; interleaved well-formed logs of 1 KiB bodies, and the same with 1 % conflicts, which change nothing below;
 * wall-clock, nine repetitions, a path wins where its median is below the other's minimum; "device path" = the log
 * (40 bytes per PATCH) and the offsets from host memory to the device, the call, a synchronise; "host path" = the
 * host twin, then extents, first and the reset states to the device, a synchronise):
 *   - 65 536 x 4, 262 144 x 4, 4096 x 64 and 1 048 576 x 1 uploads x PATCHes: the DEVICE path, at 0.14, 0.063, 0.35
 *     and 0.037 of the host path's time -- 0.37 ms against 2.8, 1.07 against 17.8, 0.35 against 1.04 and 1.25 ms
 *     against 34.5;
 *   - ONE upload owning all 1 048 576 PATCHes: the HOST path, 3.7 ms against 17.4: the wavefront's 16 384 dependent
 *     steps take about 1 us each.  A caller with one enormous upload in its log uses the twin;
 *   - the call alone, device time: 62, 165, 130 and 221 us on the four shapes (16.6 ms on the degenerate one), three
 *     to five times efes_objects_jobs behind it (22 to 44 us) and 0.1 to 0.4 of the wide walk (158 to 1727 us);
 *   - the zero-length slots are NOT free in the walk: over a table with 10 % refused PATCHes efes_hash_chain_wide
 *     takes 1.91, 1.73, 1.42 and 1.68 times what it takes over the same table compacted on the host (300 us against
 *     157, 814 against 471, 2253 against 1586, 923 against 550).  Compacting needs a count back from the device in
 *     front of the builder; a caller whose logs are full of refusals may prefer that. */
#define EFES_PATCH_LENGTH_UNKNOWN (~(uint64_t)0) /* no efes-file-length header: Go's -1 */

typedef struct efes_patch {        /* one PATCH request; the log is in ARRIVAL order */
    uint64_t data_offset;          /* its body lies at data + data_offset */
    uint64_t length;               /* body bytes: n of io.Copy (filereceiver.go:209) */
    uint64_t file_offset;          /* efes-file-offset */
    uint64_t file_length;          /* efes-file-length, or EFES_PATCH_LENGTH_UNKNOWN */
    uint32_t object;               /* upload index, < nobjects */
    uint32_t _reserved;
} efes_patch;                      /* 40 bytes */

typedef struct efes_patch_answer { /* per PATCH, arrival order */
    uint64_t offset;               /* the efes-file-offset header of the answer */
    uint32_t verdict;              /* EFES_PATCH_* */
    uint32_t slot;                 /* the extent slot this PATCH has in the table */
} efes_patch_answer;               /* 16 bytes */

typedef struct efes_patch_object { /* per object */
    uint64_t offset;               /* FileInfo.Offset after the log */
    uint32_t flags;                /* EFES_PATCH_OBJ_* */
    uint32_t admitted;             /* PATCHes of it that were admitted */
} efes_patch_object;               /* 16 bytes */

typedef struct efes_patches {      /* a HOST struct of device addresses (host addresses for the twin) */
    const efes_patch* log;             /* npatches */
    const uint64_t*   offsets;         /* nobjects: FileInfo.Offset before the log; NULL = all 0 */
    efes_sha1_state*  sha1;            /* nobjects or NULL: states of RESTARTED objects are re-initialised */
    efes_crc32_state* crc32;           /* nobjects or NULL: likewise */
    efes_extent*      extents;         /* out, npatches */
    uint32_t*         first;           /* out, nobjects + 1 */
    efes_patch_answer* answers;        /* out, npatches, or NULL */
    efes_patch_object* objects;        /* out, nobjects, or NULL */
    uint32_t*         patch_of;        /* out, npatches, or NULL: slot -> arrival index */
    uint32_t*         counts;          /* out, 5 words, or NULL: PATCHes per verdict */
    uint32_t nobjects, npatches;
} efes_patches;                    /* 88 bytes */

#define EFES_PATCH_ADMITTED 0u  /* hashed; answer.offset = the new offset; .info is saved */
#define EFES_PATCH_CONFLICT 1u  /* 409; answer.offset = the required offset */
#define EFES_PATCH_DEFERRED 2u  /* not decided in this log: resubmit it in the next, in the same order */
#define EFES_PATCH_DONE     3u  /* admitted and Offset == file_length: digests at sums + 24 * slot, .info goes */
#define EFES_PATCH_INVALID  4u  /* object >= nobjects */

#define EFES_PATCH_OBJ_RESTARTED 0x1u /* a PATCH at offset 0 was admitted: the states were re-initialised */
#define EFES_PATCH_OBJ_DONE      0x2u /* a PATCH of it was DONE */
#define EFES_PATCH_OBJ_DEFERRED  0x4u /* a PATCH of it was deferred */

size_t efes_patches_table_scratch(uint32_t nobjects, uint32_t npatches);
int efes_patches_table(efes_ctx* ctx, const efes_patches* in, void* scratch_device, size_t scratch_bytes, void* stream);
int efes_patches_table_host(const efes_patches* in);

/* Test hooks are declared in efes_testing.h: exported, but not part of the stable surface. */

/* Pure text codecs on plain states (no device work). */
void efes_sha1_state_marshal_text(const efes_sha1_state* s, char out[200]);
int efes_sha1_state_unmarshal_text(efes_sha1_state* s, const char* text, size_t n);
void efes_crc32_state_marshal_text(const efes_crc32_state* s, char out[8]);
int efes_crc32_state_unmarshal_text(efes_crc32_state* s, const char* text, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* EFES_HASH_H */
