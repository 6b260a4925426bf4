"""Python host layer over the C ABI: the reference's digest surface, GPU-backed.

Mirrors the Go types of putdotio/efes that uploads stream through:
  * ``Sha1Digest``  <- sha1digest  (sha1.go:29-120) + MarshalText/UnmarshalText (sha1_efes.go:25-64)
  * ``CRC32Digest`` <- crc32digest (crc32.go:48-93) + MarshalText/UnmarshalText (crc32_efes.go:18-40)
  * ``Sha1File``    <- Sha1File    (sha1file.go:9-53)
  * ``new_sha1`` / ``new_crc32_ieee`` <- NewSha1 (sha1.go:48) / NewCRC32IEEE (crc32.go:68)
  * ``Digest`` / ``FileInfo`` JSON  <- fileinfo.go:10-58 (the resumable `<path>.info` state)
Method names follow Python style (write/sum/marshal_text); argument meaning, return values
and error behaviour follow Go: ``write`` returns len(p); ``sum(b)`` appends the digest to b
and leaves the state untouched; ``unmarshal_text`` raises ``EfesError`` with
EFES_ERR_INVALID_DIGEST where Go returns errInvalidDigest; where the Go code would panic
the call raises ``EfesError`` with EFES_ERR_STATE.

All hashing runs on the GPU (libefeshash.so); this module only moves bytes.
"""
from __future__ import annotations

import ctypes
import io
import json
import threading

import numpy as np

from ._lib import MODE_AUTO, EfesError, Infos, Objects, ObjectsOut, PairStats, Patches, Plan, QueueStats, Results, Sha1State, check, lib

__all__ = ["Context", "default_context", "device_count", "open_devices", "crc32_combine", "crc32_batch_scratch", "crc32_chain_scratch", "crc32_copy_scratch", "hash_chain_scratch", "hash_chain_auto_mode", "hash_chain_auto_mode_wide", "objects_jobs_scratch", "objects_jobs_host", "objects_results_scratch", "objects_results_host", "objects_order_scratch", "objects_order_host", "objects_jobs_ordered_scratch", "objects_jobs_ordered_host", "infos_unmarshal_text_host", "infos_marshal_text_host", "patches_table_scratch", "patches_table_host", "Sha1Digest", "CRC32Digest", "Sha1File", "Digest", "FileInfo",
           "new_sha1", "new_crc32_ieee", "EfesError"]


def plan_batch(lengths, ctx: "Context | None" = None) -> tuple[np.ndarray, Plan]:
    """efes_plan_batch: order[i] = index of the i-th longest job; plan = split + deep shape.

    Host-only; without a context the capacity of one MI355X (1024 SIMDs) is assumed.
    """
    lengths = np.ascontiguousarray(lengths, dtype=np.uint64)
    order = np.zeros(lengths.size, dtype=np.uint32)
    plan = Plan()
    check(lib().efes_plan_batch(ctx.handle if ctx else None, lengths.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                lengths.size, order.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(plan)),
          "efes_plan_batch")
    return order, plan


def crc32_batch_scratch(n: int) -> int:
    """efes_crc32_batch_scratch: device bytes efes_crc32_batch needs for n jobs (0 for n == 0 or more
    than EFES_CRC_BATCH_MAX_JOBS)."""
    return int(lib().efes_crc32_batch_scratch(n))


def crc32_chain_scratch(n: int) -> int:
    """efes_crc32_chain_scratch: device bytes efes_crc32_chain needs for n jobs (0 for n == 0 or more
    than EFES_CRC_BATCH_MAX_JOBS; never less than crc32_batch_scratch(n))."""
    return int(lib().efes_crc32_chain_scratch(n))


def crc32_copy_scratch(n: int) -> int:
    """efes_crc32_copy_scratch: device bytes efes_crc32_copy needs for n jobs (0 for n == 0 or more than
    EFES_CRC_BATCH_MAX_JOBS; never less than crc32_chain_scratch(n))."""
    return int(lib().efes_crc32_copy_scratch(n))


def hash_chain_scratch(n: int) -> int:
    """efes_hash_chain_scratch: device bytes efes_hash_chain needs for n jobs (0 for n == 0 or more than
    EFES_HASH_CHAIN_MAX_JOBS)."""
    return int(lib().efes_hash_chain_scratch(n))


def hash_chain_auto_mode(nchains: int, ctx: "Context | None" = None) -> int:
    """efes_hash_chain_auto_mode: the mode for hash_chain_mode() when nchains objects are walked at once
    (host-only; without a context one MI355X is assumed): MODE_DEEP up to one chain per SIMD, then the
    grouped walk with as many lanes per chain as still hold every chain at once."""
    return int(lib().efes_hash_chain_auto_mode(ctx.handle if ctx else None, nchains))


def hash_chain_auto_mode_wide(nchains: int, ctx: "Context | None" = None) -> int:
    """efes_hash_chain_auto_mode_wide: hash_chain_auto_mode() for a caller that also has hash_chain_wide():
    MODE_WIDE from the measured chain count upwards (that result goes to hash_chain_wide()), else what
    hash_chain_auto_mode() gives (that goes to hash_chain_mode()).  Host-only."""
    return int(lib().efes_hash_chain_auto_mode_wide(ctx.handle if ctx else None, nchains))


def objects_jobs_scratch(nobjects: int, nextents: int) -> int:
    """efes_objects_jobs_scratch: device bytes efes_objects_jobs needs for a table of nobjects objects and
    nextents extents (0 where either exceeds EFES_OBJECTS_MAX)."""
    return int(lib().efes_objects_jobs_scratch(nobjects, nextents))


def objects_jobs_host(table: Objects, out: ObjectsOut) -> None:
    """efes_objects_jobs_host: objects_jobs() on the host -- extents, first, copy_offsets and every array of
    `out` are host addresses; the base addresses in `table` are only added to.  Needs no GPU."""
    check(lib().efes_objects_jobs_host(ctypes.byref(table), ctypes.byref(out)), "efes_objects_jobs_host")


def objects_results_scratch(nobjects: int, nextents: int) -> int:
    """efes_objects_results_scratch: device bytes efes_objects_results needs for a table of nobjects objects and
    nextents extents (0 where either exceeds EFES_OBJECTS_MAX, never 0 otherwise)."""
    return int(lib().efes_objects_results_scratch(nobjects, nextents))


def objects_results_host(table: Objects, req: Results) -> None:
    """efes_objects_results_host: objects_results() on the host -- first, sums and status of `table` and every
    array of `req` are host addresses.  Needs no GPU."""
    check(lib().efes_objects_results_host(ctypes.byref(table), ctypes.byref(req)), "efes_objects_results_host")


def objects_order_scratch(nobjects: int, nextents: int) -> int:
    """efes_objects_order_scratch: device bytes efes_objects_order needs for a table of nobjects objects and
    nextents extents (0 where either exceeds EFES_OBJECTS_MAX, never 0 otherwise)."""
    return int(lib().efes_objects_order_scratch(nobjects, nextents))


def objects_order_host(table: Objects, order_ptr: int | None) -> None:
    """efes_objects_order_host: objects_order() on the host -- extents and first of `table` and the nobjects
    32-bit words at order_ptr are host addresses.  Needs no GPU."""
    check(lib().efes_objects_order_host(ctypes.byref(table), order_ptr), "efes_objects_order_host")


def objects_jobs_ordered_scratch(nobjects: int, nextents: int) -> int:
    """efes_objects_jobs_ordered_scratch: device bytes efes_objects_jobs_ordered needs for a table of nobjects
    objects and nextents extents (0 where either exceeds EFES_OBJECTS_MAX, never 0 otherwise)."""
    return int(lib().efes_objects_jobs_ordered_scratch(nobjects, nextents))


def objects_jobs_ordered_host(table: Objects, out: ObjectsOut, order_ptr: int | None, job_first_ptr: int | None = None) -> None:
    """efes_objects_jobs_ordered_host: objects_jobs_ordered() on the host -- the arrays of objects_jobs_host(), the
    nobjects words of the order and the nobjects + 1 words of job_first (or None) are host addresses."""
    check(lib().efes_objects_jobs_ordered_host(ctypes.byref(table), ctypes.byref(out), order_ptr, job_first_ptr),
          "efes_objects_jobs_ordered_host")


def infos_unmarshal_text_host(infos: Infos) -> None:
    """efes_infos_unmarshal_text_host: Context.infos_unmarshal_text() on the host -- every array of `infos` is a host
    address, the texts at any alignment.  Needs no GPU."""
    check(lib().efes_infos_unmarshal_text_host(ctypes.byref(infos)), "efes_infos_unmarshal_text_host")


def infos_marshal_text_host(infos: Infos) -> None:
    """efes_infos_marshal_text_host: Context.infos_marshal_text() on the host.  Needs no GPU."""
    check(lib().efes_infos_marshal_text_host(ctypes.byref(infos)), "efes_infos_marshal_text_host")


def patches_table_scratch(nobjects: int, npatches: int) -> int:
    """efes_patches_table_scratch: scratch bytes Context.patches_table needs (never 0; 0 above EFES_OBJECTS_MAX)."""
    return int(lib().efes_patches_table_scratch(nobjects, npatches))


def patches_table_host(patches: Patches) -> None:
    """efes_patches_table_host: Context.patches_table() on the host -- every array of `patches` is a host address.
    Needs no GPU."""
    check(lib().efes_patches_table_host(ctypes.byref(patches)), "efes_patches_table_host")


class Context:
    """efes_ctx: one GPU, its CRC tables, one stream."""

    def __init__(self, device: int = 0):
        h = ctypes.c_void_p()
        check(lib().efes_ctx_create(device, ctypes.byref(h)), "efes_ctx_create")
        self.handle = h
        self.device = device

    @property
    def stream(self) -> int:
        return lib().efes_ctx_stream(self.handle) or 0

    def submit(self, jobs_ptr: int, njobs: int, stream: int | None = None, mode: int = MODE_AUTO) -> None:
        check(lib().efes_hash_submit_mode(self.handle, jobs_ptr, njobs, stream, mode), "efes_hash_submit")

    def plan(self, lengths) -> tuple[np.ndarray, Plan]:
        """efes_plan_batch for this context's GPU: (longest-first order, plan)."""
        return plan_batch(lengths, self)

    def submit_plan(self, jobs_ptr: int, plan: Plan, stream: int | None = None) -> None:
        """efes_hash_submit_plan: a batch laid out in plan order (DEEP part on the side stream)."""
        check(lib().efes_hash_submit_plan(self.handle, jobs_ptr, ctypes.byref(plan), stream), "efes_hash_submit_plan")

    def sync(self, stream: int | None = None) -> None:
        check(lib().efes_sync(self.handle, stream), "efes_sync")

    def fill_synthetic(self, ptr: int, nbytes: int, seed: int, stream: int | None = None) -> None:
        check(lib().efes_fill_synthetic(self.handle, ptr, nbytes, seed & 0xFFFFFFFFFFFFFFFF, stream),
              "efes_fill_synthetic")

    def crc32_span(self, data_ptr: int, nbytes: int, crc_state_ptr: int, stream: int | None = None) -> None:
        """efes_crc32_span: crc32.go Write (76-86) of one long device buffer into the device CRC state
        at crc_state_ptr, segment-parallel over the whole GPU (asynchronous on `stream`)."""
        check(lib().efes_crc32_span(self.handle, data_ptr, nbytes, crc_state_ptr, stream), "efes_crc32_span")

    def crc32_batch(self, jobs_ptr: int, njobs: int, scratch_ptr: int, scratch_bytes: int,
                    stream: int | None = None) -> None:
        """efes_crc32_batch: the CRC-only jobs (sha1 == NULL) of a device job array, their bytes dealt
        to the whole GPU in tiles; scratch: crc32_batch_scratch(njobs) device bytes, 16-byte aligned,
        one buffer per call that may overlap another (asynchronous on `stream`)."""
        check(lib().efes_crc32_batch(self.handle, jobs_ptr, njobs, scratch_ptr, scratch_bytes, stream), "efes_crc32_batch")

    def crc32_chain(self, jobs_ptr: int, njobs: int, scratch_ptr: int, scratch_bytes: int,
                    stream: int | None = None) -> None:
        """efes_crc32_chain: efes_crc32_batch that honours EFES_JOB_CHAIN -- a flagged job is the next
        Write into the state of the job before it, so one object may lie in many extents; scratch:
        crc32_chain_scratch(njobs) device bytes, otherwise as for crc32_batch."""
        check(lib().efes_crc32_chain(self.handle, jobs_ptr, njobs, scratch_ptr, scratch_bytes, stream), "efes_crc32_chain")

    def crc32_copy(self, jobs_ptr: int, dst_ptr: int, njobs: int, scratch_ptr: int, scratch_bytes: int,
                   stream: int | None = None) -> None:
        """efes_crc32_copy: crc32_chain() that also copies each job's bytes, in the same pass over them, to
        the device pointer dst[j] of the device array at dst_ptr (any alignment; 0: hashed, not copied);
        scratch: crc32_copy_scratch(njobs) device bytes, otherwise as for crc32_chain."""
        check(lib().efes_crc32_copy(self.handle, jobs_ptr, dst_ptr, njobs, scratch_ptr, scratch_bytes, stream), "efes_crc32_copy")

    def hash_chain(self, jobs_ptr: int, njobs: int, scratch_ptr: int, scratch_bytes: int,
                   stream: int | None = None) -> None:
        """efes_hash_chain: fused, SHA-1-only or CRC-only jobs as for submit(), with EFES_JOB_CHAIN honoured
        -- a flagged job is the next Write into the states of the job before it, and one wavefront walks
        each chain, so an object in many extents takes one call; scratch: hash_chain_scratch(njobs) device
        bytes, 16-byte aligned, one buffer per call that may overlap another (asynchronous on `stream`)."""
        check(lib().efes_hash_chain(self.handle, jobs_ptr, njobs, scratch_ptr, scratch_bytes, stream), "efes_hash_chain")

    def hash_chain_mode(self, jobs_ptr: int, njobs: int, scratch_ptr: int, scratch_bytes: int,
                        stream: int | None, mode: int) -> None:
        """efes_hash_chain_mode: hash_chain() with the walk chosen by the caller -- MODE_DEEP is the wave
        walk of hash_chain(), MODE_GROUP[G] the grouped walk with 64/G chains per wavefront, for more
        chains than SIMDs (hash_chain_auto_mode(nchains) picks one).  The same bytes either way; no
        MODE_AUTO, since the chain count lives on the device."""
        check(lib().efes_hash_chain_mode(self.handle, jobs_ptr, njobs, scratch_ptr, scratch_bytes, stream, mode),
              "efes_hash_chain_mode")

    def hash_chain_checkpoints(self, jobs_ptr: int, njobs: int, ckpt_ptr: int, scratch_ptr: int, scratch_bytes: int,
                               stream: int | None, mode: int) -> None:
        """efes_hash_chain_checkpoints: hash_chain_mode() that also leaves the resumable state after every
        member that asks for one -- ckpt_ptr is a device array of njobs device pointers to 112-byte
        records (CHECKPOINT_DTYPE; 0: none for that job), each written with the chain's SHA-1 state and
        CRC after that member's Write.  Everything else as hash_chain_mode(), byte for byte."""
        check(lib().efes_hash_chain_checkpoints(self.handle, jobs_ptr, njobs, ckpt_ptr, scratch_ptr, scratch_bytes,
                                                stream, mode), "efes_hash_chain_checkpoints")

    def hash_chain_wide(self, jobs_ptr: int, njobs: int, ckpt_ptr: int | None, scratch_ptr: int, scratch_bytes: int,
                        stream: int | None = None) -> None:
        """efes_hash_chain_wide: hash_chain() by the wide walk, one chain per lane, for very many chains of
        short members.  The arguments in the C call's order; ckpt_ptr None (NULL): no records; else a device array of njobs record pointers as
        for hash_chain_checkpoints().  The same bytes as hash_chain() / hash_chain_checkpoints(MODE_DEEP)."""
        check(lib().efes_hash_chain_wide(self.handle, jobs_ptr, njobs, ckpt_ptr, scratch_ptr, scratch_bytes, stream),
              "efes_hash_chain_wide")

    def hash_chain_wide_copy(self, jobs_ptr: int, njobs: int, dst_ptr: int, ckpt_ptr: int | None, scratch_ptr: int,
                             scratch_bytes: int, stream: int | None = None) -> None:
        """efes_hash_chain_wide_copy: hash_chain_wide() that also copies every member whose Write takes effect, in
        the pass that hashes it, to the device pointer dst[j] of the device array at dst_ptr (any alignment; 0:
        hashed, not copied).  ckpt_ptr, the scratch and everything written as for hash_chain_wide()."""
        check(lib().efes_hash_chain_wide_copy(self.handle, jobs_ptr, dst_ptr, ckpt_ptr, njobs, scratch_ptr, scratch_bytes,
                                              stream), "efes_hash_chain_wide_copy")

    def objects_jobs(self, table: Objects, out: ObjectsOut, scratch_ptr: int | None, scratch_bytes: int,
                     stream: int | None = None) -> None:
        """efes_objects_jobs: the object table `table` (extents and object boundaries in device memory, the base
        addresses of data, states, sums, statuses, records and the gather destination) expanded on the device
        into the job array, dst[] and ckpt[] of `out`, and the gather layout; asynchronous on `stream`, so a
        chain call queued behind it on the same stream needs no synchronisation in between."""
        check(lib().efes_objects_jobs(self.handle, ctypes.byref(table), ctypes.byref(out), scratch_ptr, scratch_bytes,
                                      stream), "efes_objects_jobs")

    def objects_order(self, table: Objects, order_ptr: int | None, scratch_ptr: int | None, scratch_bytes: int,
                      stream: int | None = None) -> None:
        """efes_objects_order: the longest-first ranking of the objects of `table` (only its extents' lengths, its
        first[] and its counts are read) into the nobjects 32-bit words at the device address order_ptr --
        descending byte size, equal sizes in ascending table index --, sorted on the device; asynchronous on
        `stream`; scratch: objects_order_scratch(nobjects, nextents) device bytes, 16-byte aligned."""
        check(lib().efes_objects_order(self.handle, ctypes.byref(table), order_ptr, scratch_ptr, scratch_bytes, stream),
              "efes_objects_order")

    def objects_jobs_ordered(self, table: Objects, out: ObjectsOut, order_ptr: int | None, job_first_ptr: int | None,
                             scratch_ptr: int | None, scratch_bytes: int, stream: int | None = None) -> None:
        """efes_objects_jobs_ordered: objects_jobs() with the objects emitted in the order of the nobjects 32-bit
        words at the device address order_ptr (objects_order()'s, or the caller's own permutation); job_first_ptr:
        None, or nobjects + 1 device words for the first slot of every rank.  What the walks write stays in table
        order; scratch: objects_jobs_ordered_scratch(nobjects, nextents) device bytes."""
        check(lib().efes_objects_jobs_ordered(self.handle, ctypes.byref(table), ctypes.byref(out), order_ptr, job_first_ptr,
                                              scratch_ptr, scratch_bytes, stream), "efes_objects_jobs_ordered")

    def objects_results(self, table: Objects, req: Results, scratch_ptr: int | None, scratch_bytes: int,
                        stream: int | None = None) -> None:
        """efes_objects_results: from the object table `table` (the one objects_jobs() was given) and the sums and
        statuses a chain call left behind it, one 32-byte result per object (digest, status, verdict against
        req.expected under req.compare), the ascending list of the objects whose verdict is MISMATCH or FAILED,
        and the four verdict counters, all in device memory; asynchronous on `stream`, so queued behind the chain
        call on the same stream it needs no synchronisation in between."""
        check(lib().efes_objects_results(self.handle, ctypes.byref(table), ctypes.byref(req), scratch_ptr, scratch_bytes,
                                         stream), "efes_objects_results")

    def checkpoints_marshal_text(self, ckpt_ptr: int, n: int, text_ptr: int, stream: int | None = None) -> None:
        """efes_checkpoints_marshal_text: the `.info` texts of n contiguous device records at ckpt_ptr,
        CHECKPOINT_TEXT_BYTES characters each at text_ptr (device): the 200 of the SHA-1 state's
        MarshalText, then the 8 of the CRC's (asynchronous on `stream`)."""
        check(lib().efes_checkpoints_marshal_text(self.handle, ckpt_ptr, n, text_ptr, stream),
              "efes_checkpoints_marshal_text")

    def infos_unmarshal_text(self, infos: Infos, stream: int | None = None) -> None:
        """efes_infos_unmarshal_text: the n `.info` records at infos.text (208 characters each, device memory)
        decoded into the states at infos.sha1 and infos.crc32; a record with a character that is no hex digit leaves
        the refusing state (nx = EFES_SHA1_NX_REFUSED), CRC 0 and status EFES_ERR_INVALID_DIGEST, and is counted in
        infos.counts[1].  Asynchronous on `stream`, so the builder and a walk queue directly behind it."""
        check(lib().efes_infos_unmarshal_text(self.handle, ctypes.byref(infos), stream), "efes_infos_unmarshal_text")

    def infos_marshal_text(self, infos: Infos, stream: int | None = None) -> None:
        """efes_infos_marshal_text: the states at infos.sha1 and infos.crc32 (zeros for one that is None) encoded
        into n `.info` records at infos.text, 208 lower-case characters each (asynchronous on `stream`)."""
        check(lib().efes_infos_marshal_text(self.handle, ctypes.byref(infos), stream), "efes_infos_marshal_text")

    def patches_table(self, patches: Patches, scratch_ptr: int | None, scratch_bytes: int, stream: int | None = None) -> None:
        """efes_patches_table: the arrival log of PATCH records at patches.log sorted by upload and run through
        saveFile's admission rules on the device: the object table (extents, first) that objects_jobs takes as it
        is, the answer of every PATCH, the new offset of every upload, and fresh states for restarted uploads.
        Asynchronous on `stream`, so the builder and a walk queue directly behind it."""
        check(lib().efes_patches_table(self.handle, ctypes.byref(patches), scratch_ptr, scratch_bytes, stream), "efes_patches_table")

    def debug_fault_after(self, k: int) -> None:
        """Test hook (efes_debug_fault_after): the k-th launch of this context's digest queue faults."""
        check(lib().efes_debug_fault_after(self.handle, k), "efes_debug_fault_after")

    def debug_set_cus(self, cus: int) -> None:
        """Test hook (efes_debug_set_cus): this context's launchers size their grids for `cus` compute units,
        1 <= cus <= the device's own count (which restores it).  Fewer workgroups, nothing else."""
        check(lib().efes_debug_set_cus(self.handle, cus), "efes_debug_set_cus")

    def copy_to_host(self, dst_host: int, src_device: int, nbytes: int, stream: int | None = None) -> None:
        check(lib().efes_copy_to_host(self.handle, dst_host, src_device, nbytes, stream), "efes_copy_to_host")

    def copy_to_device(self, dst_device: int, src_host: int, nbytes: int, stream: int | None = None) -> None:
        check(lib().efes_copy_to_device(self.handle, dst_device, src_host, nbytes, stream), "efes_copy_to_device")

    def close(self) -> None:
        if self.handle:
            lib().efes_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):  # pragma: no cover - interpreter teardown order
        try:
            self.close()
        except Exception:
            pass


_ctx_lock = threading.Lock()
_contexts: dict[int, Context] = {}


def default_context(device: int = 0) -> Context:
    with _ctx_lock:
        if device not in _contexts:
            _contexts[device] = Context(device)
        return _contexts[device]


class Pool:
    """efes_pool (ABI 5): digests spread over several contexts (one process over every GPU,
    server.go:130).  Each digest takes its upload slot, at every (re)open, on the context whose
    digest queue has the most free slots."""

    def __init__(self, ctxs):
        self.ctxs = list(ctxs)
        arr = (ctypes.c_void_p * len(self.ctxs))(*[c.handle.value for c in self.ctxs])
        h = ctypes.c_void_p()
        check(lib().efes_pool_create(arr, len(self.ctxs), ctypes.byref(h)), "efes_pool_create")
        self.handle = h
        self._mu = threading.Lock()
        self._live = 0  # digests made on the pool and not yet freed
        self._closing = False

    def _adopt(self) -> None:  # a digest is being made on the pool
        with self._mu:
            if self._closing or not self.handle:
                raise EfesError(-4, "pool closed")
            self._live += 1

    def _release(self) -> None:  # a digest of the pool was freed
        with self._mu:
            self._live -= 1
            last = self._closing and self._live == 0
        if last:
            self._destroy()

    def _destroy(self) -> None:
        if self.handle:
            lib().efes_pool_destroy(self.handle)
            self.handle = None

    def stats(self, i: int) -> QueueStats:
        """Counters of the digest queue of context i (efes_pool_stats)."""
        st = QueueStats()
        check(lib().efes_pool_stats(self.handle, i, ctypes.byref(st)), "efes_pool_stats")
        return st

    def close(self) -> None:
        """efes_pool_destroy -- deferred until the last digest made on the pool is freed (the C pool
        must outlive its digests: a Write of a live digest re-reads the pool's contexts)."""
        with self._mu:
            self._closing = True
            now = self._live == 0
        if now:
            self._destroy()


def device_count() -> int:
    """efes_device_count (ABI 7): HIP devices the process sees, of any architecture (0 without any)."""
    return int(lib().efes_device_count())


def open_devices(devices=None) -> tuple[list[Context], list[tuple[int, str]]]:
    """The contexts of go/hash_gpu.go's pool(): one per ordinal of `devices` (default: every ordinal
    below device_count()), skipping -- never stopping at -- the ones whose efes_ctx_create fails.
    Returns (contexts that opened, [(ordinal, reason) of each one skipped])."""
    ctxs, skipped = [], []
    for dev in (range(device_count()) if devices is None else devices):
        try:
            ctxs.append(Context(int(dev)))
        except EfesError as e:
            skipped.append((int(dev), strerror_of(e.code)))
    return ctxs, skipped


def strerror_of(code: int) -> str:
    return lib().efes_strerror(code).decode()


def pair_stats() -> dict:
    """efes_pair_stats_get (ABI 6): process-wide counters of fused CRC + SHA-1 digest pairs."""
    st = PairStats()
    check(lib().efes_pair_stats_get(ctypes.byref(st)), "efes_pair_stats_get")
    return {f: int(getattr(st, f)) for f, _ in PairStats._fields_}


def crc32_combine(crc1: int, crc2: int, len2: int) -> int:
    """CRC-32 of A||B from crc(A), crc(B), |B| (efes_crc32_combine; crc32.go is GF(2)-linear)."""
    return int(lib().efes_crc32_combine(crc1 & 0xFFFFFFFF, crc2 & 0xFFFFFFFF, len2))


def _as_bytes(p) -> bytes:
    if isinstance(p, str):
        return p.encode()
    return bytes(p)


class Sha1Digest:
    """sha1digest (sha1.go:29-34) whose compressions run on the GPU."""

    def __init__(self, ctx: Context | None = None, reset: bool = True, pool: Pool | None = None):
        h = ctypes.c_void_p()
        if pool is not None:  # the pool must outlive its digests: keep a reference, count this one
            self.ctx, self.pool = None, None
            pool._adopt()
            fn = lib().efes_sha1_new_pool if reset else lib().efes_sha1_new_zero_pool
            rc = fn(pool.handle, ctypes.byref(h))
            if rc:
                pool._release()
            check(rc, "efes_sha1_new_pool")
            self.pool = pool
        else:
            self.ctx, self.pool = ctx or default_context(), None
            fn = lib().efes_sha1_new if reset else lib().efes_sha1_new_zero
            check(fn(self.ctx.handle, ctypes.byref(h)), "efes_sha1_new")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            lib().efes_sha1_free(self._h)
            self._h = None
            if getattr(self, "pool", None) is not None:
                self.pool._release()

    def reset(self) -> None:  # sha1.go:36-44
        lib().efes_sha1_reset(self._h)

    def size(self) -> int:  # sha1.go:54
        return lib().efes_sha1_size()

    def block_size(self) -> int:  # sha1.go:56
        return lib().efes_sha1_block_size()

    def write(self, p) -> int:  # sha1.go:58-79
        b = _as_bytes(p)
        check(lib().efes_sha1_write(self._h, b, len(b)), "Sha1Digest.write")
        return len(b)

    def sum(self, b: bytes = b"") -> bytes:  # sha1.go:82-87
        out = (ctypes.c_uint8 * 20)()
        check(lib().efes_sha1_sum(self._h, out), "Sha1Digest.sum")
        return bytes(b) + bytes(out)

    def hexdigest(self) -> str:
        return self.sum().hex()

    def marshal_text(self) -> bytes:  # sha1_efes.go:25-38
        out = ctypes.create_string_buffer(200)
        check(lib().efes_sha1_marshal_text(self._h, out), "Sha1Digest.marshal_text")
        return out.raw[:200]

    def unmarshal_text(self, text) -> None:  # sha1_efes.go:40-64
        t = _as_bytes(text)
        check(lib().efes_sha1_unmarshal_text(self._h, t, len(t)), "Sha1Digest.unmarshal_text")

    def state(self) -> Sha1State:
        st = Sha1State()
        check(lib().efes_sha1_get_state(self._h, ctypes.byref(st)), "Sha1Digest.state")
        return st

    def set_state(self, st: Sha1State) -> None:
        check(lib().efes_sha1_set_state(self._h, ctypes.byref(st)), "Sha1Digest.set_state")


class CRC32Digest:
    """crc32digest (crc32.go:48-51) with the IEEE table, updated on the GPU."""

    def __init__(self, ctx: Context | None = None, pool: Pool | None = None):
        h = ctypes.c_void_p()
        if pool is not None:
            self.ctx, self.pool = None, None
            pool._adopt()
            rc = lib().efes_crc32_new_pool(pool.handle, ctypes.byref(h))
            if rc:
                pool._release()
            check(rc, "efes_crc32_new_pool")
            self.pool = pool
        else:
            self.ctx, self.pool = ctx or default_context(), None
            check(lib().efes_crc32_new(self.ctx.handle, ctypes.byref(h)), "efes_crc32_new")
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            lib().efes_crc32_free(self._h)
            self._h = None
            if getattr(self, "pool", None) is not None:
                self.pool._release()

    def reset(self) -> None:  # crc32.go:74
        lib().efes_crc32_reset(self._h)

    def size(self) -> int:  # crc32.go:70
        return lib().efes_crc32_size()

    def block_size(self) -> int:  # crc32.go:72
        return lib().efes_crc32_block_size()

    def write(self, p) -> int:  # crc32.go:76-86
        b = _as_bytes(p)
        check(lib().efes_crc32_write(self._h, b, len(b)), "CRC32Digest.write")
        return len(b)

    def sum32(self) -> int:  # crc32.go:88
        v = ctypes.c_uint32()
        check(lib().efes_crc32_sum32(self._h, ctypes.byref(v)), "CRC32Digest.sum32")
        return v.value

    def sum(self, b: bytes = b"") -> bytes:  # crc32.go:90-93
        return bytes(b) + self.sum32().to_bytes(4, "big")

    def marshal_text(self) -> bytes:  # crc32_efes.go:18-24
        out = ctypes.create_string_buffer(8)
        check(lib().efes_crc32_marshal_text(self._h, out), "CRC32Digest.marshal_text")
        return out.raw[:8]

    def unmarshal_text(self, text) -> None:  # crc32_efes.go:26-40
        t = _as_bytes(text)
        check(lib().efes_crc32_unmarshal_text(self._h, t, len(t)), "CRC32Digest.unmarshal_text")


def new_sha1(ctx: Context | None = None, pool: Pool | None = None) -> Sha1Digest:  # sha1.go:48-52 NewSha1
    return Sha1Digest(ctx, pool=pool)


def new_crc32_ieee(ctx: Context | None = None, pool: Pool | None = None) -> CRC32Digest:  # crc32.go:68
    return CRC32Digest(ctx, pool=pool)


class Sha1File(io.RawIOBase):
    """sha1file.go:9-53: hashes a ReadSeeker's bytes as they are read, once each.

    ``read`` hashes only bytes beyond what was already hashed (so a retry after a seek
    back does not double-hash); reading while positioned past the hashed prefix raises
    IOError("missing data for sha1"); ``seek`` forward raises IOError("seeking forward
    is not supported") after the underlying seek, exactly as the Go code does.
    """

    def __init__(self, rs, ctx: Context | None = None):  # sha1file.go:16-21
        super().__init__()
        self.rs = rs
        self.position = 0
        self.calculated = 0
        self.digest = new_sha1(ctx)

    def readable(self) -> bool:
        return True

    def seekable(self) -> bool:
        return True

    def read(self, n: int = -1) -> bytes:  # sha1file.go:23-37
        if self.position > self.calculated:
            raise IOError("missing data for sha1")
        prev = self.position
        p = self.rs.read(n)
        self.position += len(p)
        if self.position > self.calculated:
            crop = self.calculated - prev
            c = p[crop:]
            self.digest.write(c)
            self.calculated += len(c)
        return p

    def readinto(self, b) -> int:
        p = self.read(len(b))
        b[:len(p)] = p
        return len(p)

    def seek(self, offset: int, whence: int = io.SEEK_SET) -> int:  # sha1file.go:39-49
        new_position = self.rs.seek(offset, whence)
        if self.position < new_position:
            raise IOError("seeking forward is not supported")
        self.position = new_position
        return new_position

    def tell(self) -> int:
        return self.position

    def sum(self, b: bytes = b"") -> bytes:  # sha1file.go:51-53
        return self.digest.sum(b)


class Digest:
    """fileinfo.go:15-18 `Digest{Sha1 *sha1digest "sha1"; CRC32 *crc32digest "crc32"}`."""

    def __init__(self, ctx: Context | None = None, pool: Pool | None = None):
        self.sha1 = new_sha1(ctx, pool)
        self.crc32 = new_crc32_ieee(ctx, pool)

    def write(self, p) -> int:
        """filereceiver.go:208 io.MultiWriter(f, CRC32, Sha1): CRC first, then SHA-1."""
        self.crc32.write(p)
        return self.sha1.write(p)

    def to_json(self) -> dict:
        return {"sha1": self.sha1.marshal_text().decode(), "crc32": self.crc32.marshal_text().decode()}

    def load_json(self, d: dict) -> None:
        self.sha1.unmarshal_text(d["sha1"])
        self.crc32.unmarshal_text(d["crc32"])


class FileInfo:
    """fileinfo.go:10-13 `FileInfo{Offset "offset"; Digest "digest"}` and its JSON file codec."""

    def __init__(self, ctx: Context | None = None, pool: Pool | None = None):  # fileinfo.go:20-27 newFileInfo
        self.offset = 0
        self.digest = Digest(ctx, pool)

    def dumps(self) -> str:  # fileinfo.go:47-58 json.NewEncoder(f).Encode(fi)
        return json.dumps({"offset": self.offset, "digest": self.digest.to_json()}, separators=(",", ":")) + "\n"

    @classmethod
    def loads(cls, s: str, ctx: Context | None = None, pool: Pool | None = None) -> "FileInfo":  # fileinfo.go:37-45
        d = json.loads(s)
        fi = cls(ctx, pool)
        fi.offset = int(d["offset"])
        fi.digest.load_json(d["digest"])
        return fi
