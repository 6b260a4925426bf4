"""Device-resident batches of independent jobs (layer 1 of include/efes_hash.h).

A batch is N independent `Write(p)` (+ Sum) jobs over messages that already live in
device memory -- the shape of many concurrent uploads (filereceiver.go:208-209, one
request goroutine per upload).  Device buffers are torch tensors (plumbing only); the
hashing is libefeshash.so.
"""
from __future__ import annotations

import numpy as np

from ._lib import (CHECKPOINT_DTYPE, CHECKPOINT_TEXT_BYTES, EFES_HASH_CRC32, EFES_HASH_SHA1, EFES_INFO_TEXT_BYTES, EFES_OBJECTS_FRESH, EFES_OBJECTS_RUNNING, EFES_JOB_CHAIN, EFES_JOB_FINALIZE, EFES_JOB_INIT, EFES_JOB_SUM_ONLY, JOB_DTYPE, MODE_AUTO, MODE_DEEP, MODE_FED4,
                   MODE_FED4E, MODE_GROUP, MODE_WIDE, OBJECT_RESULT_DTYPE, PATCH_ANSWER_DTYPE, PATCH_DTYPE, PATCH_OBJECT_DTYPE, PLAN_MAX_PARTS, SHA1_STATE_DTYPE, Infos, Objects, ObjectsOut, Patches, Plan, PlanPart,
                   Results)
from .hashing import Context, crc32_batch_scratch, crc32_chain_scratch, crc32_copy_scratch, default_context, hash_chain_auto_mode, hash_chain_auto_mode_wide, hash_chain_scratch, objects_jobs_ordered_scratch, objects_jobs_scratch, objects_order_scratch, objects_results_scratch, patches_table_scratch

MODE_PLAN = -1  # run(): efes_plan_batch + efes_hash_submit_plan instead of one fixed kernel shape

# lanes per job -> kernel shape, in forced_plan's spec (64 = DEEP, 0 = WIDE, 1 = FED4, 2 = FED4E)
_SPEC_MODES = {64: MODE_DEEP, 0: MODE_WIDE, 1: MODE_FED4, 2: MODE_FED4E, **MODE_GROUP}


def forced_plan(n: int, spec: str) -> Plan:
    """A caller-built efes_plan (efes_hash.h lets a caller place its own parts) for n longest-first
    jobs: "<lanes>:<jobs>[x],..." -- lanes 64 = DEEP, 0 = WIDE, 1 = FED4, 2 = FED4E (both always own
    their CUs), 4/8/16/32 = GROUPn; x = exclusive (CUs of its own) -- in order, the jobs beyond the
    listed parts WIDE.  Raises ValueError for an unknown shape or more than PLAN_MAX_PARTS parts."""
    parts, used = [], 0
    for item in filter(None, spec.split(",")):
        lanes, _, jobs = item.partition(":")
        excl = jobs.endswith("x")
        if int(lanes) not in _SPEC_MODES:
            raise ValueError(f"unknown shape {lanes!r}")
        take = min(int(jobs.rstrip("x")), n - used)
        if take:
            parts.append((take, _SPEC_MODES[int(lanes)], excl))
        used += take
    if used < n:
        parts.append((n - used, MODE_WIDE, False))
    if len(parts) > PLAN_MAX_PARTS:
        raise ValueError(f"{len(parts)} parts > {PLAN_MAX_PARTS}")
    plan = Plan()
    plan.njobs, plan.nparts = n, len(parts)
    for i, (j, m, x) in enumerate(parts):
        plan.part[i] = PlanPart(j, m, 1 if x else 0, 0)
    return plan

IV = np.array([0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0], dtype=np.uint32)


def fresh_states(n: int) -> np.ndarray:
    """n states equal to NewSha1() (sha1.go:48-52)."""
    st = np.zeros(n, dtype=SHA1_STATE_DTYPE)
    st["h"][:] = IV
    return st


class DeviceBatch:
    """Jobs j = 0..N-1: Write(data[offsets[j] : offsets[j]+lengths[j]]) into state j (+ Sum).

    Kernels run on torch's current stream.  When that is the null stream (handle 0, which
    efes_hash.h maps to the context's own non-blocking stream), submit() orders the context
    stream after the work torch queued so far and torch's stream after the launch, so
    reset() / result reads on torch's stream stay ordered with the kernels either way.
    """

    def __init__(self, data_ptr: int, offsets, lengths, *, sha1: bool = True, crc32: bool = True,
                 finalize: bool = True, fresh: bool = False, states: np.ndarray | None = None, crcs: np.ndarray | None = None,
                 ctx: Context | None = None, device: str = "cuda:0", sum_only: bool = False):
        import torch

        self.ctx = ctx or default_context(int(device.split(":")[1]) if ":" in device else 0)
        self.torch = torch
        self.device = device
        offsets = np.asarray(offsets, dtype=np.uint64)
        lengths = np.asarray(lengths, dtype=np.uint64)
        n = self.n = int(offsets.size)
        assert lengths.size == n
        self.has_sha1 = bool(sha1)
        self._crc_scratch = None  # submit_crc_batch()'s device scratch, allocated once
        self.init_states = fresh_states(n) if states is None else np.array(states, dtype=SHA1_STATE_DTYPE)
        self.init_crcs = np.zeros(n, np.uint32) if crcs is None else np.asarray(crcs, dtype=np.uint32)
        self._init_states_dev = torch.from_numpy(self.init_states.view(np.uint8).copy()).to(device)
        self._init_crcs_dev = torch.from_numpy(self.init_crcs.view(np.uint8).copy()).to(device)
        self.states = self._init_states_dev.clone()
        self.crcs = self._init_crcs_dev.clone()
        self.sums = torch.zeros(max(n, 1) * 24, dtype=torch.uint8, device=device)
        self.status = torch.full((max(n, 1),), -99, dtype=torch.int32, device=device)
        jobs = np.zeros(n, dtype=JOB_DTYPE)
        jobs["data"] = np.uint64(data_ptr) + offsets
        jobs["length"] = lengths
        if sha1:
            jobs["sha1"] = np.uint64(self.states.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(104)
        if crc32:
            jobs["crc32"] = np.uint64(self.crcs.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4)
        if finalize:
            jobs["sum"] = np.uint64(self.sums.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(24)
            jobs["flags"] |= EFES_JOB_FINALIZE
        if fresh:  # new chunks: start from NewSha1()/NewCRC32IEEE(), in-states are not read
            jobs["flags"] |= EFES_JOB_INIT
        if sum_only:  # Sum of the in-states on a copy (sha1.go:82-87): states are not written
            assert finalize and not lengths.any(), "sum_only jobs are zero-length FINALIZE jobs"
            jobs["flags"] |= EFES_JOB_SUM_ONLY
        jobs["status"] = np.uint64(self.status.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(4)
        self.jobs_host = jobs
        self.jobs = torch.from_numpy(jobs.view(np.uint8).copy()).to(device)
        torch.cuda.synchronize(device)

    def variant(self, *, fresh: bool, finalize: bool) -> "DeviceBatch":
        """The same jobs over the same data, states, sums and status with other flags: one segment
        of a resumed Write sequence (EFES_JOB_INIT on the first segment, EFES_JOB_FINALIZE on the
        last; the states stay in HBM between them, filereceiver.go:182-226)."""
        import copy

        v = copy.copy(self)
        jobs = self.jobs_host.copy()
        jobs["flags"] &= np.uint32(~(EFES_JOB_INIT | EFES_JOB_FINALIZE) & 0xFFFFFFFF)
        if fresh:
            jobs["flags"] |= EFES_JOB_INIT
        if finalize:
            assert int(self.jobs_host["sum"][0]) != 0, "a finalizing variant needs a batch made with finalize=True"
            jobs["flags"] |= EFES_JOB_FINALIZE
        v.jobs_host = jobs
        v.jobs = self.torch.from_numpy(jobs.view(np.uint8).copy()).to(self.device)
        if hasattr(v, "plan"):
            del v.plan
        self.torch.cuda.synchronize(self.device)
        return v

    def stream(self) -> int:
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def reset(self) -> None:
        """Restore the initial states (async, on torch's current stream)."""
        self.states.copy_(self._init_states_dev)
        self.crcs.copy_(self._init_crcs_dev)

    def submit(self, mode: int = MODE_AUTO) -> None:
        """Enqueue all jobs, ordered after the work on torch's current stream (data writes,
        reset()) and before the work queued there afterwards (result copies)."""
        self._ordered(lambda stream: self._launch(mode, stream))

    def _ordered(self, launch) -> None:
        """launch(stream handle), ordered with torch's current stream as submit() documents."""
        cur = self.torch.cuda.current_stream(self.device)
        if cur.cuda_stream:
            launch(cur.cuda_stream)
            return
        # Null stream: the library launches on the context's non-blocking stream, which the
        # null stream does not order against; join the two both ways with events.
        ctx_stream = self.torch.cuda.ExternalStream(self.ctx.stream, device=self.device)
        ctx_stream.wait_stream(cur)
        launch(ctx_stream.cuda_stream)
        cur.wait_stream(ctx_stream)

    def submit_crc_batch(self) -> None:
        """The jobs of a batch built with sha1=False through efes_crc32_batch (every job's bytes dealt
        to the whole GPU in tiles) instead of the job kernels; ordered exactly like submit().  The
        scratch tensor is allocated on first use and kept: one batch's launches run in stream order."""
        if self.has_sha1:
            raise ValueError("submit_crc_batch: the batch carries SHA-1 states (build it with sha1=False)")
        if self._crc_scratch is None:
            self._crc_scratch = self.torch.empty(max(crc32_batch_scratch(self.n), 16), dtype=self.torch.uint8,
                                                 device=self.device)
        self._ordered(lambda stream: self.ctx.crc32_batch(self.jobs.data_ptr(), self.n, self._crc_scratch.data_ptr(),
                                                          self._crc_scratch.numel(), stream))

    def run_crc_batch(self) -> None:
        self.submit_crc_batch()
        self.torch.cuda.synchronize(self.device)

    def _launch(self, mode: int, stream: int) -> None:
        if mode == MODE_PLAN:
            if not hasattr(self, "plan"):
                self.make_plan()
            self.ctx.submit_plan(self.jobs_planned.data_ptr(), self.plan, stream)
        else:
            self.ctx.submit(self.jobs.data_ptr(), self.n, stream, mode)

    def run(self, mode: int = MODE_AUTO) -> None:
        self.submit(mode)
        self.torch.cuda.synchronize(self.device)

    def make_plan(self, force: str | None = None) -> None:
        """efes_plan_batch over the job lengths; keeps a longest-first copy of the job array.  `force`
        replaces the planner's parts by caller-built ones (forced_plan) over the same order."""
        order, self.plan = self.ctx.plan(self.jobs_host["length"])
        if force is not None:
            self.plan = forced_plan(self.n, force)
        self.jobs_planned = self.torch.from_numpy(self.jobs_host[order].view(np.uint8).copy()).to(self.device)
        self.torch.cuda.synchronize(self.device)

    def submit_planned(self) -> None:
        """The planned launch (DEEP/grouped part concurrent with the WIDE part), ordered like submit()."""
        self.submit(MODE_PLAN)

    # ---- results (host copies)
    def status_host(self) -> np.ndarray:
        return self.status.cpu().numpy()[: self.n]

    def sums_host(self) -> np.ndarray:
        return self.sums.cpu().numpy()[: self.n * 24].reshape(self.n, 24)

    def sha1_hex(self) -> list[str]:
        s = self.sums_host()
        return [bytes(r[:20]).hex() for r in s]

    def crc_sum(self) -> np.ndarray:
        return self.crcs.cpu().numpy().view(np.uint32)[: self.n]

    def states_host(self) -> np.ndarray:
        return self.states.cpu().numpy().view(SHA1_STATE_DTYPE)[: self.n]


COPY_ALIGN = 256  # DeviceObjects(copy_to=...): every object's start in the default layout


def default_copy_offsets(objects) -> tuple[np.ndarray, int]:
    """The default destination layout of DeviceObjects(copy_to=...): the objects back to back in their
    order, every object's start rounded up to COPY_ALIGN bytes.  Host arithmetic over the extents'
    lengths: (offset of each object, bytes of room the layout needs)."""
    sizes = [sum(int(n) for _, n in o) for o in objects]
    offsets, at = np.zeros(len(sizes), dtype=np.uint64), 0
    for i, size in enumerate(sizes):
        at = (at + COPY_ALIGN - 1) // COPY_ALIGN * COPY_ALIGN
        offsets[i] = at
        at += size
    return offsets, at


class DeviceObjects:
    """CRC-32 (and, with sha1=True, SHA-1) of objects that lie in many device extents, in one call:
    efes_crc32_chain for the default CRC-only set, efes_hash_chain for a set built with sha1=True.

    objects[i] is a list of (offset, length) extents of the buffer at data_ptr, in the object's byte
    order: one job per extent and one state per object, the first extent's job the chain's head
    (with EFES_JOB_INIT when `fresh`, else starting from crcs[i]), the others with EFES_JOB_CHAIN.
    EFES_JOB_FINALIZE goes on the last extent of each object, or on every extent when `running` (the
    CRC after each extent, what `.info` holds after each PATCH).  An object without extents takes no
    job and keeps its in-state.  Ordered with torch's current stream as DeviceBatch is.

    sha1=True keeps one 104-byte SHA-1 state per object as well (NewSha1(), or states[i]) and hashes
    through efes_hash_chain, one wavefront per object: fused with crc32=True, SHA-1 alone with
    crc32=False.  Then sha1_hex() is the Sum at each object's last extent, running_sha1() the Sum at
    every extent's end (running=True) and states_host() the states, stale tail bytes included.

    walk (sha1=True only) chooses how efes_hash_chain walks the objects: None is efes_hash_chain itself,
    one wavefront per object; "auto" is efes_hash_chain_mode at the mode efes_hash_chain_auto_mode gives
    for the number of objects that have extents (the grouped walk beyond one object per SIMD); an
    EFES_MODE_* constant is passed to efes_hash_chain_mode as it is.  "wide" submits through
    efes_hash_chain_wide, one object per lane, for very many objects of short extents; "auto_wide" does so
    where efes_hash_chain_auto_mode_wide gives EFES_MODE_WIDE for the number of objects that have extents,
    and is "auto" below that.  The results are the same bytes.

    copy_to (CRC-only sets) also gathers the objects, in the pass that hashes them, through
    efes_crc32_copy: each object's extents are written one behind the other, in the object's byte order,
    starting at the device address copy_to + copy_offsets[i].  The default copy_offsets are those of
    default_copy_offsets(objects); .copy_offsets holds the offsets in use and .copy_bytes the room they
    need behind copy_to.  The destination must not overlap the source, the states or the sums.
    With sha1=True only the wide walk copies: walk="wide" with copy_to gathers by the same layout rules
    through efes_hash_chain_wide_copy (with crc32=False and with checkpoints=True too); every other walk,
    "auto_wide" included, which may resolve to a grouped walk, raises ValueError.

    checkpoints=True (sha1=True only; a CRC-only set's running CRCs already are its checkpoints) also
    keeps one 112-byte record per extent, contiguous in extent order, and always submits through
    efes_hash_chain_checkpoints -- at the mode `walk` gives ("auto" as above), EFES_MODE_DEEP without one --
    or, with the wide walk, through efes_hash_chain_wide with its record pointers.
    checkpoints_host() is the records (the resumable SHA-1 state and the CRC after each extent),
    checkpoint_texts() their `.info` texts, marshalled on the device.

    build chooses where the job array, the destination pointers and the record pointers are made.  "host"
    (the default) fills them with numpy and uploads them, up to 72 bytes per extent.  "device" uploads the
    compact object table instead -- 16 bytes per extent, 4 per object -- and lets efes_objects_jobs expand it
    on torch's current stream; the constructor then does not wait for the device, submit() may follow at
    once, and jobs, _dst, _ckpt_ptrs, copy_offsets and copy_bytes hold the same bytes and values as with
    "host" (copy_offsets, copy_bytes and jobs_host are read back from the device on first use).
    from_table() builds the set from a table that already lies in device memory.

    order (build="device" and from_table() only; anything but "table" with build="host" raises ValueError) chooses
    the order of the objects in the job array, which decides how the walks draw them.  "table" (the default) is
    the table's own; "longest_first" ranks the objects by byte size on the device (efes_objects_order) and emits
    them in that order (efes_objects_jobs_ordered), on torch's current stream with no wait; a device tensor of
    nobjects 32-bit integers is the caller's own permutation.  What the walks write is in TABLE order whatever
    the job order, so every accessor returns what it returns for "table"; order_host() is the permutation,
    job_first_host() the slots of every rank and jobs_host the records in slot order.  Measured on shuffled
    tables, "longest_first" made no walk faster and two slower (efes_hash.h "Object order"): it is for a caller
    that wants that order for its own reasons, not a default.

    infos (instead of states= and crcs=; implies fresh=False) resumes every object from its `.info` texts, decoded ON
    THE DEVICE (efes_infos_unmarshal_text) into the initial states on torch's current stream, in front of the builder
    and with no wait: a device uint8 tensor of nobjects x 208 characters (info_texts(device=True) of an earlier
    round), a host (nobjects, 208) uint8 array, or a list of (sha1_text, crc32_text) byte pairs.  A text with a
    character that is no hex digit -- a pair of the wrong length becomes a row of b"?" -- leaves the REFUSING state:
    that object's members all get EFES_ERR_STATE, nothing of it is gathered, results() gives EFES_VERDICT_FAILED,
    and the other objects run.  A CRC-only set has no refusing state: the CRC of a broken text starts from 0, so
    such a caller reads resume_counts() or resume_status_host() before it trusts the CRCs.  reset() restores the
    decoded states without decoding again.  info_texts() marshals the states every object has NOW (after a run: the
    texts its `.info` holds next) on the device, for every set, with or without checkpoints=True.

    verify(expected) and results() sort the per-extent sums and statuses out per object ON THE DEVICE
    (efes_objects_results): verdicts against expected digests, the ascending list of the objects that are not in
    order and four counters, of which verify() copies only the counters and the list to the host.
    """

    _ordered = DeviceBatch._ordered

    def __init__(self, data_ptr: int, objects, *, crcs: np.ndarray | None = None, fresh: bool | None = None,
                 running: bool = False, ctx: Context | None = None, device: str = "cuda:0", sha1: bool = False,
                 crc32: bool = True, states: np.ndarray | None = None, walk=None, copy_to: int | None = None,
                 copy_offsets=None, checkpoints: bool = False, build: str = "host", order="table", infos=None):
        if build not in ("host", "device"):
            raise ValueError(f'DeviceObjects: build={build!r} (build="host" or build="device")')
        objects = [list(o) for o in objects]
        fresh, infos = DeviceObjects._check_infos(infos, fresh, states, crcs, len(objects))
        DeviceObjects._check_order(order, build)
        if checkpoints and not sha1:
            raise ValueError("DeviceObjects: checkpoints= needs sha1=True (a CRC-only set's running CRCs are its checkpoints)")
        if copy_to is not None and sha1 and not (isinstance(walk, str) and walk == "wide"):
            raise ValueError('DeviceObjects: copy_to= with sha1=True needs walk="wide" (efes_hash_chain_wide_copy): no other '
                             "walk copies; copy_to= is otherwise CRC-only (efes_crc32_copy): build the set with sha1=False")
        if copy_offsets is not None and copy_to is None:
            raise ValueError("DeviceObjects: copy_offsets= needs copy_to=")
        import torch

        if not (sha1 or crc32):
            raise ValueError("DeviceObjects: sha1 or crc32 (or both)")
        if walk is not None and not sha1:
            raise ValueError("DeviceObjects: walk= needs sha1=True")
        if states is not None and not sha1:
            raise ValueError("DeviceObjects: states= needs sha1=True")
        self.has_sha1, self.has_crc32 = bool(sha1), bool(crc32)
        self.build = build

        self.ctx = ctx or default_context(int(device.split(":")[1]) if ":" in device else 0)
        self.torch = torch
        self.device = device
        self.nobjects = len(objects)
        counts = np.array([len(o) for o in objects], dtype=np.int64)
        n = self.n = int(counts.sum())
        self.first = np.concatenate(([0], np.cumsum(counts)))[:-1] if self.nobjects else np.zeros(0, np.int64)
        self.last = self.first + counts - 1  # job of each object's last extent (first - 1: no extents)
        ext = np.array([e for o in objects for e in o], dtype=np.uint64).reshape(n, 2)
        if build == "device":  # the compact table goes up; efes_objects_jobs makes the arrays below
            bounds = np.concatenate(([0], np.cumsum(counts))).astype(np.uint32)
            offs = None if copy_offsets is None else np.ascontiguousarray(copy_offsets, dtype=np.uint64)
            assert offs is None or offs.size == self.nobjects
            self._build_on_device(data_ptr, torch.from_numpy(ext.view(np.int64)).to(device),
                                  torch.from_numpy(bounds.view(np.int32)).to(device), int((counts > 0).sum()), crcs=crcs,
                                  fresh=fresh, running=running, states=states, walk=walk, copy_to=copy_to,
                                  copy_offsets=None if offs is None else torch.from_numpy(offs.view(np.int64)).to(device),
                                  checkpoints=checkpoints, order=order, infos=infos)
            return
        owner = np.repeat(np.arange(self.nobjects, dtype=np.uint64), counts)
        if infos is not None:
            self._resume_from_infos(infos)
        else:
            self.init_crcs = np.zeros(self.nobjects, np.uint32) if crcs is None else np.asarray(crcs, dtype=np.uint32)
            assert self.init_crcs.size == self.nobjects
            self._init_crcs_dev = torch.from_numpy(self.init_crcs.view(np.uint8).copy()).to(device)
        self.crcs = self._init_crcs_dev.clone() if self.nobjects else torch.zeros(4, dtype=torch.uint8, device=device)
        self.sums = torch.zeros(max(n, 1) * 24, dtype=torch.uint8, device=device)
        self.status = torch.full((max(n, 1),), -99, dtype=torch.int32, device=device)
        idx = np.arange(n, dtype=np.uint64)
        jobs = np.zeros(n, dtype=JOB_DTYPE)
        jobs["data"] = np.uint64(data_ptr) + ext[:, 0]
        jobs["length"] = ext[:, 1]
        if crc32:
            jobs["crc32"] = np.uint64(self.crcs.data_ptr()) + owner * np.uint64(4)
        if sha1:
            if infos is None:
                self.init_states = fresh_states(self.nobjects) if states is None else np.array(states, dtype=SHA1_STATE_DTYPE)
                assert self.init_states.size == self.nobjects
                self._init_states_dev = torch.from_numpy(self.init_states.view(np.uint8).copy()).to(device)
            self.states = self._init_states_dev.clone() if self.nobjects else torch.zeros(104, dtype=torch.uint8, device=device)
            jobs["sha1"] = np.uint64(self.states.data_ptr()) + owner * np.uint64(104)
        jobs["sum"] = np.uint64(self.sums.data_ptr()) + idx * np.uint64(24)
        jobs["status"] = np.uint64(self.status.data_ptr()) + idx * np.uint64(4)
        jobs["flags"] = EFES_JOB_CHAIN
        heads = self.first[counts > 0]
        jobs["flags"][heads] = EFES_JOB_INIT if fresh else 0
        if running:
            jobs["flags"] |= EFES_JOB_FINALIZE
        else:
            jobs["flags"][self.last[counts > 0]] |= EFES_JOB_FINALIZE
        self.running = bool(running)
        self.wide, self.walk = self._resolve_walk(walk, int((counts > 0).sum()))
        self.jobs_host = jobs
        self.jobs = torch.from_numpy(jobs.view(np.uint8).copy()).to(device) if n else torch.zeros(56, dtype=torch.uint8, device=device)
        self.has_checkpoints = bool(checkpoints)
        if checkpoints:  # one record per extent, ckpt[j] = base + 112 j
            if self.walk is None:
                self.walk = MODE_DEEP
            self.ckpt = torch.zeros(max(n, 1) * CHECKPOINT_DTYPE.itemsize, dtype=torch.uint8, device=device)
            at = np.uint64(self.ckpt.data_ptr()) + idx * np.uint64(CHECKPOINT_DTYPE.itemsize)
            self._ckpt_ptrs = torch.from_numpy(at.astype(np.uint64).view(np.uint8).copy()).to(device) if n else torch.zeros(8, dtype=torch.uint8, device=device)
        # allocated once and kept: one object set's launches run in stream order
        scratch_bytes = hash_chain_scratch(n) if sha1 else crc32_chain_scratch(n)
        self.copy_to = copy_to
        if copy_to is not None:
            sizes = np.array([sum(int(m) for _, m in o) for o in objects], dtype=np.uint64)
            if copy_offsets is None:
                self.copy_offsets, self.copy_bytes = default_copy_offsets(objects)
            else:
                self.copy_offsets = np.asarray(copy_offsets, dtype=np.uint64)
                assert self.copy_offsets.size == self.nobjects
                self.copy_bytes = int((self.copy_offsets + sizes).max()) if self.nobjects else 0
            # each extent behind the extents before it in its object
            before = np.cumsum(ext[:, 1]) - ext[:, 1]
            within = before - before[self.first[owner.astype(np.int64)]] if n else before
            dst = np.uint64(copy_to) + self.copy_offsets[owner.astype(np.int64)] + within
            self._dst = torch.from_numpy(dst.astype(np.uint64).view(np.uint8).copy()).to(device) if n else torch.zeros(8, dtype=torch.uint8, device=device)
            if not sha1:  # the wide walk with copy takes the chain calls' scratch
                scratch_bytes = crc32_copy_scratch(n)
        self._scratch = torch.empty(max(scratch_bytes, 16), dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)

    @classmethod
    def from_table(cls, data_ptr: int, extents, first, *, crcs: np.ndarray | None = None, fresh: bool | None = None,
                   running: bool = False, ctx: Context | None = None, device: str = "cuda:0", sha1: bool = False,
                   crc32: bool = True, states: np.ndarray | None = None, walk=None, copy_to: int | None = None,
                   copy_offsets=None, checkpoints: bool = False, order="table", infos=None) -> "DeviceObjects":
        """The set of an object table that already lies in DEVICE memory: `extents`, a contiguous torch tensor of
        shape (n, 2) of 64-bit integers, (offset, length) per extent, and `first`, one of shape (nobjects + 1,)
        of 32-bit integers, object i owning the extents [first[i], first[i + 1]).  The other arguments are the
        constructor's; copy_offsets, where given, is a device tensor of nobjects 64-bit integers.  The table is
        never copied to the host while the set is built or submitted (efes_objects_jobs expands it in stream
        order); first, last, copy_offsets and copy_bytes are fetched when first read, which sha1_hex() does.
        walk="auto" and "auto_wide" need the number of objects that have extents on the host and raise
        ValueError: pass "wide", None or an EFES_MODE_* constant.  order as for the constructor: "longest_first"
        ranks the objects on the device, so a table straight from a device-side pool is walked longest first
        without ever visiting the host.  infos as for the constructor: with a device tensor of texts neither the
        table nor the states ever visit the host."""
        DeviceObjects._check_order(order, "device")
        if checkpoints and not sha1:
            raise ValueError("DeviceObjects: checkpoints= needs sha1=True (a CRC-only set's running CRCs are its checkpoints)")
        if copy_to is not None and sha1 and not (isinstance(walk, str) and walk == "wide"):
            raise ValueError('DeviceObjects: copy_to= with sha1=True needs walk="wide" (efes_hash_chain_wide_copy)')
        if copy_offsets is not None and copy_to is None:
            raise ValueError("DeviceObjects: copy_offsets= needs copy_to=")
        if not (sha1 or crc32):
            raise ValueError("DeviceObjects: sha1 or crc32 (or both)")
        if (walk is not None or states is not None) and not sha1:
            raise ValueError("DeviceObjects: walk= and states= need sha1=True")
        if isinstance(walk, str) and walk in ("auto", "auto_wide"):
            raise ValueError(f'DeviceObjects.from_table: walk={walk!r} needs the chain count on the host')
        if extents.dim() != 2 or extents.shape[1] != 2 or extents.element_size() != 8 or not extents.is_contiguous():
            raise ValueError("DeviceObjects.from_table: extents is a contiguous (n, 2) tensor of 64-bit integers")
        if first.dim() != 1 or first.numel() < 1 or first.element_size() != 4 or not first.is_contiguous():
            raise ValueError("DeviceObjects.from_table: first is a contiguous (nobjects + 1,) tensor of 32-bit integers")
        fresh, infos = DeviceObjects._check_infos(infos, fresh, states, crcs, int(first.numel()) - 1)
        import torch

        self = cls.__new__(cls)
        self.has_sha1, self.has_crc32 = bool(sha1), bool(crc32)
        self.build = "device"
        self.ctx = ctx or default_context(int(device.split(":")[1]) if ":" in device else 0)
        self.torch = torch
        self.device = device
        self.nobjects, self.n = int(first.numel()) - 1, int(extents.shape[0])
        self._build_on_device(data_ptr, extents, first, None, crcs=crcs, fresh=fresh, running=running, states=states,
                              walk=walk, copy_to=copy_to, copy_offsets=copy_offsets, checkpoints=checkpoints, order=order,
                              infos=infos)
        return self

    @classmethod
    def from_patches(cls, data_ptr: int, log, offsets=None, *, nobjects: int | None = None, infos=None,
                     states: np.ndarray | None = None, crcs: np.ndarray | None = None, sha1: bool = False, crc32: bool = True,
                     walk=None, running: bool = False, checkpoints: bool = False, copy_to: int | None = None, order="table",
                     ctx: Context | None = None, device: str = "cuda:0") -> "DeviceObjects":
        """The set of an ARRIVAL LOG of PATCH requests: `log`, a host PATCH_DTYPE array or a device tensor of
        npatches x 40 bytes, in arrival order and interleaved over the uploads as a server receives them, and
        `offsets`, the FileInfo.Offset every upload has before the log (a host array or a device tensor of nobjects
        64-bit integers; None: all 0).  efes_patches_table sorts the log by upload and applies saveFile's rules on
        torch's current stream -- behind the initial states (states=, crcs= or infos=, as for the constructor;
        without them NewSha1() and CRC 0) and in front of the builder, with no wait anywhere -- so the set is the
        table of the ADMITTED PATCHes: one slot per PATCH, a refused one of length 0.  The uploads never start
        fresh: each resumes from its state, which the call re-initialises for an upload that a PATCH at offset 0
        restarts; reset() restores the states with those restarts applied.  nobjects is taken from offsets, infos,
        states or crcs, whichever is given, else it must be passed.  walk="auto" and "auto_wide" raise as for
        from_table().  patch_answers_host() is what every PATCH is answered with (verdict, efes-file-offset and
        slot, in arrival order), patch_objects_host() every upload's new offset, flags and admitted count,
        patch_counts() the PATCHes per verdict and patch_of_host() the arrival index of every slot.  With
        running=True the digests of a DONE PATCH are running_sha1()[slot] and running_crcs()[slot] of its answer's slot."""
        if hasattr(log, "data_ptr"):
            if log.element_size() * int(log.numel()) % PATCH_DTYPE.itemsize or not log.is_contiguous():
                raise ValueError("DeviceObjects.from_patches: log is a contiguous device tensor of npatches x 40 bytes")
            npatches = log.element_size() * int(log.numel()) // PATCH_DTYPE.itemsize
        else:
            log = np.ascontiguousarray(log)
            if log.dtype != PATCH_DTYPE or log.ndim != 1:
                raise ValueError("DeviceObjects.from_patches: log is a one-dimensional PATCH_DTYPE array (or a device tensor)")
            npatches = int(log.size)
        for given in (offsets, states, crcs):
            if nobjects is None and given is not None:
                nobjects = int(given.numel()) if hasattr(given, "data_ptr") else int(np.asarray(given).shape[0])
        if nobjects is None and infos is not None:
            nobjects = int(infos.numel()) // EFES_INFO_TEXT_BYTES if hasattr(infos, "data_ptr") else len(infos)
        if nobjects is None:
            raise ValueError("DeviceObjects.from_patches: nobjects= (or offsets=, infos=, states= or crcs=, which give it)")
        if offsets is not None and (int(offsets.numel()) if hasattr(offsets, "data_ptr") else int(np.asarray(offsets).size)) != nobjects:
            raise ValueError(f"DeviceObjects.from_patches: offsets has not {nobjects} entries")
        DeviceObjects._check_order(order, "device")
        if checkpoints and not sha1:
            raise ValueError("DeviceObjects: checkpoints= needs sha1=True (a CRC-only set's running CRCs are its checkpoints)")
        if copy_to is not None and sha1 and not (isinstance(walk, str) and walk == "wide"):
            raise ValueError('DeviceObjects: copy_to= with sha1=True needs walk="wide" (efes_hash_chain_wide_copy)')
        if not (sha1 or crc32):
            raise ValueError("DeviceObjects: sha1 or crc32 (or both)")
        if (walk is not None or states is not None) and not sha1:
            raise ValueError("DeviceObjects: walk= and states= need sha1=True")
        if isinstance(walk, str) and walk in ("auto", "auto_wide"):
            raise ValueError(f'DeviceObjects.from_patches: walk={walk!r} needs the chain count on the host')
        _, infos = DeviceObjects._check_infos(infos, False, states, crcs, nobjects)
        import torch

        self = cls.__new__(cls)
        self.has_sha1, self.has_crc32 = bool(sha1), bool(crc32)
        self.build = "device"
        self.ctx = ctx or default_context(int(device.split(":")[1]) if ":" in device else 0)
        self.torch = torch
        self.device = device
        m, n = int(nobjects), int(npatches)
        self.nobjects, self.n = m, n
        self._patch_log = log if hasattr(log, "data_ptr") else torch.from_numpy(log.view(np.uint8).reshape(-1)).to(device)
        if offsets is None or hasattr(offsets, "data_ptr"):
            self._patch_offsets = offsets
        else:
            self._patch_offsets = torch.from_numpy(np.ascontiguousarray(offsets, dtype=np.uint64).view(np.int64)).to(device)
        ext = torch.empty((n, 2), dtype=torch.int64, device=device)
        first = torch.empty(m + 1, dtype=torch.int32, device=device)
        self._patch_answers = torch.empty(max(n, 1) * PATCH_ANSWER_DTYPE.itemsize, dtype=torch.uint8, device=device)
        self._patch_objects = torch.empty(max(m, 1) * PATCH_OBJECT_DTYPE.itemsize, dtype=torch.uint8, device=device)
        self._patch_of = torch.empty(max(n, 1), dtype=torch.int32, device=device)
        self._patch_counts = torch.empty(5, dtype=torch.int32, device=device)
        self._patch_scratch = torch.empty(patches_table_scratch(m, n), dtype=torch.uint8, device=device)

        def table():  # behind the initial states, in front of their clones
            req = Patches(log=self._patch_log.data_ptr() or None,
                          offsets=None if self._patch_offsets is None else (self._patch_offsets.data_ptr() or None),
                          sha1=(self._init_states_dev.data_ptr() or None) if sha1 else None,
                          crc32=(self._init_crcs_dev.data_ptr() or None) if crc32 else None,
                          extents=ext.data_ptr() or None, first=first.data_ptr(), answers=self._patch_answers.data_ptr(),
                          objects=self._patch_objects.data_ptr(), patch_of=self._patch_of.data_ptr(),
                          counts=self._patch_counts.data_ptr(), nobjects=m, npatches=n)
            self._ordered(lambda stream: self.ctx.patches_table(req, self._patch_scratch.data_ptr(), self._patch_scratch.numel(), stream))

        self._build_on_device(data_ptr, ext, first, None, crcs=crcs, fresh=False, running=running, states=states, walk=walk,
                              copy_to=copy_to, copy_offsets=None, checkpoints=checkpoints, order=order, infos=infos,
                              before_clone=table)
        return self

    def _need_patches(self, what: str) -> None:
        if "_patch_counts" not in self.__dict__:
            raise ValueError(f"{what}: build the set with from_patches()")

    def patch_answers_host(self) -> np.ndarray:
        """Per PATCH, in arrival order: a PATCH_ANSWER_DTYPE array of (offset, verdict, slot)."""
        self._need_patches("patch_answers_host")
        return self._patch_answers.cpu().numpy()[: self.n * PATCH_ANSWER_DTYPE.itemsize].view(PATCH_ANSWER_DTYPE).copy()

    def patch_objects_host(self) -> np.ndarray:
        """Per upload: a PATCH_OBJECT_DTYPE array of (offset after the log, EFES_PATCH_OBJ_* flags, admitted PATCHes)."""
        self._need_patches("patch_objects_host")
        return self._patch_objects.cpu().numpy()[: self.nobjects * PATCH_OBJECT_DTYPE.itemsize].view(PATCH_OBJECT_DTYPE).copy()

    def patch_counts(self) -> tuple:
        """(admitted, conflict, deferred, done, invalid): the PATCHes per verdict (20 bytes read back)."""
        self._need_patches("patch_counts")
        return tuple(int(c) for c in self._patch_counts.cpu().numpy().view(np.uint32))

    def patch_of_host(self) -> np.ndarray:
        """Per slot of the table: the arrival index of its PATCH."""
        self._need_patches("patch_of_host")
        return self._patch_of.cpu().numpy().view(np.uint32)[: self.n].copy()

    @staticmethod
    def _check_infos(infos, fresh, states, crcs, nobjects: int):
        """(fresh, infos) of the infos= and fresh= arguments, checked from the arguments alone: no device is touched.
        infos comes back as None, as the caller's device tensor, or as a host (nobjects, 208) uint8 array; a list of
        (sha1_text, crc32_text) pairs is packed into one, a pair of the wrong length as a row of b"?"."""
        if infos is None:
            return (True if fresh is None else bool(fresh)), None
        if fresh:
            raise ValueError("DeviceObjects: infos= resumes the objects from their `.info` texts; fresh=True starts them anew")
        if states is not None or crcs is not None:
            raise ValueError("DeviceObjects: infos= gives the initial states; states= and crcs= do not go with it")
        want = f"DeviceObjects: infos is {nobjects} x {EFES_INFO_TEXT_BYTES} uint8 characters (a device tensor, a host array of that shape) or {nobjects} (sha1_text, crc32_text) pairs"
        if hasattr(infos, "data_ptr"):
            if str(infos.dtype) != "torch.uint8" or int(infos.numel()) != nobjects * EFES_INFO_TEXT_BYTES or not infos.is_contiguous():
                raise ValueError(f"{want} (got a {infos.dtype} tensor of shape {tuple(infos.shape)})")
            return False, infos
        if isinstance(infos, np.ndarray):
            if infos.dtype != np.uint8 or infos.shape != (nobjects, EFES_INFO_TEXT_BYTES):
                raise ValueError(f"{want} (got {infos.dtype} {infos.shape})")
            return False, np.ascontiguousarray(infos)
        pairs = list(infos)
        if len(pairs) != nobjects or any(not isinstance(p, (tuple, list)) or len(p) != 2 for p in pairs):
            raise ValueError(f"{want} (got {len(pairs)} entries)")
        rows = np.full((nobjects, EFES_INFO_TEXT_BYTES), ord("?"), np.uint8)
        for i, (a, b) in enumerate(pairs):
            a, b = (t.encode() if isinstance(t, str) else bytes(t) for t in (a, b))
            if len(a) == 200 and len(b) == 8:  # any other length: errInvalidDigest in Go, the refusing row here
                rows[i] = np.frombuffer(a + b, np.uint8)
        return False, rows

    def _resume_from_infos(self, infos) -> None:
        """The initial states decoded from the texts by efes_infos_unmarshal_text, on torch's current stream and with
        no wait: _init_crcs_dev and _init_states_dev as the other constructors leave them, so reset() restores the
        decoded states; the per-object statuses and the two counters stay on the device until asked for."""
        torch, device, m = self.torch, self.device, self.nobjects
        text = infos if hasattr(infos, "data_ptr") else torch.from_numpy(infos.reshape(-1)).to(device)
        if str(text.device) != str(torch.device(device)):
            text = text.to(device)
        if text.data_ptr() & 7:  # a view into a larger tensor: the call reads 8 characters at a time
            text = text.clone()
        self.init_crcs = self.init_states = None  # known on the device only
        self._init_crcs_dev = torch.zeros(m * 4, dtype=torch.uint8, device=device)
        if self.has_sha1:
            self._init_states_dev = torch.empty(m * SHA1_STATE_DTYPE.itemsize, dtype=torch.uint8, device=device)
        self._resume_status = torch.zeros(max(m, 1), dtype=torch.int32, device=device)
        self._resume_counts = torch.zeros(2, dtype=torch.int32, device=device)
        self._resume_text = text  # alive until the set goes: the call that reads it is only queued
        req = Infos(text=text.data_ptr() or None, sha1=(self._init_states_dev.data_ptr() or None) if self.has_sha1 else None,
                    crc32=(self._init_crcs_dev.data_ptr() or None) if self.has_crc32 else None,
                    status=self._resume_status.data_ptr(), counts=self._resume_counts.data_ptr(), n=m)
        self._ordered(lambda stream: self.ctx.infos_unmarshal_text(req, stream))

    def _need_infos(self, what: str) -> None:
        if "_resume_counts" not in self.__dict__:
            raise ValueError(f"{what}: build the set with infos=")

    def resume_counts(self) -> tuple:
        """(valid, invalid): how many of the infos= texts decoded and how many left the refusing state (8 bytes read
        back)."""
        self._need_infos("resume_counts")
        c = self._resume_counts.cpu().numpy().view(np.uint32)
        return int(c[0]), int(c[1])

    def resume_status_host(self) -> np.ndarray:
        """Per object: EFES_OK, or EFES_ERR_INVALID_DIGEST for an infos= text with a character that is no hex digit."""
        self._need_infos("resume_status_host")
        return self._resume_status.cpu().numpy()[: self.nobjects].copy()

    def info_texts(self, device: bool = False):
        """Per object: the `.info` texts of the states and CRCs the set holds now, marshalled on the device by
        efes_infos_marshal_text on torch's current stream (behind a run: what `.info` holds after this PATCH).
        device=True returns the device tensor of nobjects x 208 characters, which is a later set's infos= as it is;
        otherwise a list of (sha1_text, crc32_text) byte pairs, 200 and 8 characters, like checkpoint_texts().  A
        digest the set does not keep marshals as zeros."""
        torch, m = self.torch, self.nobjects
        text = torch.empty(m * EFES_INFO_TEXT_BYTES, dtype=torch.uint8, device=self.device)
        req = Infos(text=text.data_ptr() or None, sha1=self.states.data_ptr() if self.has_sha1 else None,
                    crc32=self.crcs.data_ptr() if self.has_crc32 else None, n=m)
        self._ordered(lambda stream: self.ctx.infos_marshal_text(req, stream))
        if device:
            return text
        rows = text.cpu().numpy().reshape(m, EFES_INFO_TEXT_BYTES)
        return [(bytes(r[:200]), bytes(r[200:])) for r in rows]

    @staticmethod
    def _check_order(order, build) -> None:
        """order= checked from the arguments alone: no device is touched."""
        if isinstance(order, str):
            if order not in ("table", "longest_first"):
                raise ValueError(f'DeviceObjects: order={order!r} (order="table", "longest_first" or a device tensor of nobjects '
                                 "32-bit integers)")
        elif not hasattr(order, "data_ptr") or order.dim() != 1 or order.element_size() != 4 or not order.is_contiguous():
            raise ValueError('DeviceObjects: order is "table", "longest_first" or a contiguous device tensor of nobjects 32-bit integers')
        if build == "host" and not (isinstance(order, str) and order == "table"):
            raise ValueError('DeviceObjects: order= other than "table" needs build="device" (the host build emits table order)')

    def _build_on_device(self, data_ptr: int, ext, first, nchains, *, crcs, fresh, running, states, walk, copy_to,
                         copy_offsets, checkpoints, order="table", infos=None, before_clone=None) -> None:
        """The rest of a set whose arrays efes_objects_jobs makes: ext, first (and copy_offsets) are device
        tensors, kept until the set goes; the states, sums, statuses and records as the host build allocates
        them; then the call on torch's current stream, with no wait behind it.  With an order other than
        "table": efes_objects_order (order="longest_first") and efes_objects_jobs_ordered instead, likewise.
        before_clone, where given, is called once the initial states lie on the device (_init_crcs_dev,
        _init_states_dev) and before they are cloned into the working states: what it queues there reaches both."""
        torch, device, n, sha1 = self.torch, self.device, self.n, self.has_sha1
        self._table_ext, self._table_first, self._table_offsets = ext, first, copy_offsets
        if infos is not None:
            self._resume_from_infos(infos)
        else:
            self.init_crcs = np.zeros(self.nobjects, np.uint32) if crcs is None else np.asarray(crcs, dtype=np.uint32)
            assert self.init_crcs.size == self.nobjects
            self._init_crcs_dev = torch.from_numpy(self.init_crcs.view(np.uint8).copy()).to(device)
            if sha1:
                self.init_states = fresh_states(self.nobjects) if states is None else np.array(states, dtype=SHA1_STATE_DTYPE)
                assert self.init_states.size == self.nobjects
                self._init_states_dev = torch.from_numpy(self.init_states.view(np.uint8).copy()).to(device)
        if before_clone is not None:
            before_clone()
        self.crcs = self._init_crcs_dev.clone() if self.nobjects else torch.zeros(4, dtype=torch.uint8, device=device)
        self.sums = torch.zeros(max(n, 1) * 24, dtype=torch.uint8, device=device)
        self.status = torch.full((max(n, 1),), -99, dtype=torch.int32, device=device)
        if sha1:
            self.states = self._init_states_dev.clone() if self.nobjects else torch.zeros(104, dtype=torch.uint8, device=device)
        self.running = bool(running)
        self.wide, self.walk = self._resolve_walk(walk, nchains)
        self.jobs = (torch.empty if n else torch.zeros)(max(n, 1) * JOB_DTYPE.itemsize, dtype=torch.uint8, device=device)
        self.has_checkpoints = bool(checkpoints)
        if checkpoints:
            if self.walk is None:
                self.walk = MODE_DEEP
            self.ckpt = torch.zeros(max(n, 1) * CHECKPOINT_DTYPE.itemsize, dtype=torch.uint8, device=device)
            self._ckpt_ptrs = (torch.empty if n else torch.zeros)(max(n, 1) * 8, dtype=torch.uint8, device=device)
        scratch_bytes = hash_chain_scratch(n) if sha1 else crc32_chain_scratch(n)
        self.copy_to = copy_to
        if copy_to is not None:
            self._dst = (torch.empty if n else torch.zeros)(max(n, 1) * 8, dtype=torch.uint8, device=device)
            self._layout = torch.zeros(self.nobjects + 1, dtype=torch.int64, device=device)
            if not sha1:
                scratch_bytes = crc32_copy_scratch(n)
        # one buffer for the builder and the walks behind it: all of them use it in stream order
        self._scratch = torch.empty(max(scratch_bytes, objects_jobs_scratch(self.nobjects, n), 16), dtype=torch.uint8, device=device)
        table = Objects(data=int(data_ptr), extents=ext.data_ptr() or None, first=first.data_ptr(),
                        sha1=self.states.data_ptr() if sha1 else None, crc32=self.crcs.data_ptr() if self.has_crc32 else None,
                        sums=self.sums.data_ptr(), status=self.status.data_ptr(),
                        ckpt=self.ckpt.data_ptr() if checkpoints else None, copy_to=None if copy_to is None else int(copy_to),
                        copy_offsets=None if copy_offsets is None else copy_offsets.data_ptr(),
                        nobjects=self.nobjects, nextents=n,
                        flags=(EFES_OBJECTS_FRESH if fresh else 0) | (EFES_OBJECTS_RUNNING if running else 0), copy_align=COPY_ALIGN)
        out = ObjectsOut(jobs=self.jobs.data_ptr(), dst=self._dst.data_ptr() if copy_to is not None else None,
                         ckpt=self._ckpt_ptrs.data_ptr() if checkpoints else None,
                         layout=self._layout.data_ptr() if copy_to is not None else None)
        if isinstance(order, str) and order == "table":
            self._ordered(lambda stream: self.ctx.objects_jobs(table, out, self._scratch.data_ptr(), self._scratch.numel(), stream))
            return
        m = self.nobjects
        rank = isinstance(order, str)  # "longest_first": the order is made here
        if not rank and int(order.numel()) != m:
            raise ValueError(f"DeviceObjects: order has {int(order.numel())} entries for {m} objects")
        need = max(objects_jobs_ordered_scratch(m, n), objects_order_scratch(m, n) if rank else 0)
        if need > self._scratch.numel():  # still one buffer for the order call, the builder and the walk behind them
            self._scratch = torch.empty(need, dtype=torch.uint8, device=device)
        self._order = torch.empty(max(m, 1), dtype=torch.int32, device=device) if rank else order
        self._job_first = torch.zeros(m + 1, dtype=torch.int32, device=device)
        if rank:
            self._ordered(lambda stream: self.ctx.objects_order(table, self._order.data_ptr(), self._scratch.data_ptr(),
                                                                self._scratch.numel(), stream))
        self._ordered(lambda stream: self.ctx.objects_jobs_ordered(table, out, self._order.data_ptr() or None, self._job_first.data_ptr(),
                                                                   self._scratch.data_ptr(), self._scratch.numel(), stream))

    def order_host(self) -> np.ndarray:
        """The permutation the job array was emitted in: order_host()[r] is the table index of the object at rank
        r (the identity for order="table").  Fetched from the device when called."""
        if "_order" in self.__dict__:
            return self._order.cpu().numpy().view(np.uint32)[: self.nobjects].copy()
        return np.arange(self.nobjects, dtype=np.uint32)

    def job_first_host(self) -> np.ndarray:
        """nobjects + 1 slot boundaries: the jobs of the object at rank r are jobs_host[job_first_host()[r] :
        job_first_host()[r + 1]] (the table's boundaries for order="table")."""
        if "_job_first" in self.__dict__:
            return self._job_first.cpu().numpy().view(np.uint32)[: self.nobjects + 1].copy()
        return np.concatenate((self.first, [self.n])).astype(np.uint32)

    _FETCHED = ("first", "last", "copy_offsets", "copy_bytes", "jobs_host")

    def __getattr__(self, name):
        """What a set built on the device leaves there until it is read: the object boundaries of from_table(),
        the gather layout, the job records."""
        d = self.__dict__
        if name in DeviceObjects._FETCHED and "_table_first" in d:
            if name in ("first", "last"):
                f = d["_table_first"].cpu().numpy().view(np.uint32).astype(np.int64)
                self.first, self.last = f[:-1], f[1:] - 1
            elif name == "jobs_host":
                self.jobs_host = self.jobs.cpu().numpy()[: self.n * JOB_DTYPE.itemsize].view(JOB_DTYPE).copy()
            elif d.get("copy_to") is not None:
                lay = d["_layout"].cpu().numpy().view(np.uint64)
                self.copy_offsets, self.copy_bytes = lay[:-1].copy(), int(lay[-1])
            if name in d:
                return d[name]
        raise AttributeError(f"{type(self).__name__!r} object has no attribute {name!r}")

    def reset(self) -> None:
        """Restore the initial states (async, on torch's current stream)."""
        if self.nobjects:
            self.crcs.copy_(self._init_crcs_dev)
            if self.has_sha1:
                self.states.copy_(self._init_states_dev)

    def _resolve_walk(self, walk, nchains: int):
        """(wide, mode) of a walk= argument: wide says that submit() calls efes_hash_chain_wide; otherwise mode
        goes to efes_hash_chain_mode (None: efes_hash_chain itself).  An EFES_MODE_* constant passes as it is,
        EFES_MODE_WIDE included, which efes_hash_chain_mode refuses."""
        if not isinstance(walk, str):
            return False, walk
        if walk == "wide":
            return True, MODE_WIDE
        if walk == "auto_wide":
            mode = hash_chain_auto_mode_wide(nchains, self.ctx)
            return mode == MODE_WIDE, mode
        if walk == "auto":
            return False, hash_chain_auto_mode(nchains, self.ctx)
        raise ValueError(f"DeviceObjects: walk={walk!r}")

    def submit(self) -> None:
        if self.wide:
            ckpt = self._ckpt_ptrs.data_ptr() if self.has_checkpoints else None
            if self.copy_to is not None:
                self._ordered(lambda stream: self.ctx.hash_chain_wide_copy(self.jobs.data_ptr(), self.n, self._dst.data_ptr(), ckpt,
                                                                           self._scratch.data_ptr(), self._scratch.numel(), stream))
                return
            self._ordered(lambda stream: self.ctx.hash_chain_wide(self.jobs.data_ptr(), self.n, ckpt, self._scratch.data_ptr(),
                                                                  self._scratch.numel(), stream))
            return
        if self.has_checkpoints:
            self._ordered(lambda stream: self.ctx.hash_chain_checkpoints(self.jobs.data_ptr(), self.n, self._ckpt_ptrs.data_ptr(),
                                                                         self._scratch.data_ptr(), self._scratch.numel(),
                                                                         stream, self.walk))
            return
        if self.walk is not None:
            self._ordered(lambda stream: self.ctx.hash_chain_mode(self.jobs.data_ptr(), self.n, self._scratch.data_ptr(),
                                                                  self._scratch.numel(), stream, self.walk))
            return
        if self.copy_to is not None:
            self._ordered(lambda stream: self.ctx.crc32_copy(self.jobs.data_ptr(), self._dst.data_ptr(), self.n,
                                                             self._scratch.data_ptr(), self._scratch.numel(), stream))
            return
        call = self.ctx.hash_chain if self.has_sha1 else self.ctx.crc32_chain
        self._ordered(lambda stream: call(self.jobs.data_ptr(), self.n, self._scratch.data_ptr(),
                                          self._scratch.numel(), stream))

    def run(self) -> None:
        self.submit()
        self.torch.cuda.synchronize(self.device)

    # ---- results (host copies)
    def status_host(self) -> np.ndarray:
        """Per extent."""
        return self.status.cpu().numpy()[: self.n]

    def crc_sum(self) -> np.ndarray:
        """Per object: the state after its last extent."""
        return self.crcs.cpu().numpy().view(np.uint32)[: self.nobjects]

    def running_crcs(self) -> np.ndarray:
        """Per extent: the object's CRC at that extent's end (a set built with running=True)."""
        if not self.running:
            raise ValueError("running_crcs: build the set with running=True")
        return self.sums.cpu().numpy()[: self.n * 24].reshape(self.n, 24)[:, 20:].copy().view(">u4").reshape(-1).astype(np.uint32)

    def _need_sha1(self, what: str) -> None:
        if not self.has_sha1:
            raise ValueError(f"{what}: build the set with sha1=True")

    def sha1_hex(self) -> list:
        """Per object: the SHA-1 Sum at its last extent's end (None for an object without extents)."""
        self._need_sha1("sha1_hex")
        s = self.sums.cpu().numpy()[: self.n * 24].reshape(self.n, 24)
        return [bytes(s[int(j), :20]).hex() if j >= f else None for f, j in zip(self.first, self.last)]

    def running_sha1(self) -> list:
        """Per extent: the object's SHA-1 Sum at that extent's end (a set built with running=True)."""
        self._need_sha1("running_sha1")
        if not self.running:
            raise ValueError("running_sha1: build the set with running=True")
        return [bytes(r[:20]).hex() for r in self.sums.cpu().numpy()[: self.n * 24].reshape(self.n, 24)]

    def states_host(self) -> np.ndarray:
        """Per object: the SHA-1 state after its last extent (h, x with its stale bytes, nx, len)."""
        self._need_sha1("states_host")
        return self.states.cpu().numpy().view(SHA1_STATE_DTYPE)[: self.nobjects]

    def _need_checkpoints(self, what: str) -> None:
        if not self.has_checkpoints:
            raise ValueError(f"{what}: build the set with sha1=True, checkpoints=True")

    def checkpoints_host(self) -> np.ndarray:
        """Per extent: the record after that extent's Write (CHECKPOINT_DTYPE: the SHA-1 state with its
        stale bytes, the CRC)."""
        self._need_checkpoints("checkpoints_host")
        return self.ckpt.cpu().numpy().view(CHECKPOINT_DTYPE)[: self.n]

    def checkpoint_texts(self) -> list:
        """Per extent: (sha1_text, crc32_text) as bytes, 200 and 8 characters, what `.info` holds after
        that extent's PATCH; marshalled on the device by efes_checkpoints_marshal_text."""
        self._need_checkpoints("checkpoint_texts")
        text = self.torch.empty(max(self.n, 1) * CHECKPOINT_TEXT_BYTES, dtype=self.torch.uint8, device=self.device)
        self._ordered(lambda stream: self.ctx.checkpoints_marshal_text(self.ckpt.data_ptr(), self.n, text.data_ptr(), stream))
        rows = text.cpu().numpy()[: self.n * CHECKPOINT_TEXT_BYTES].reshape(self.n, CHECKPOINT_TEXT_BYTES)
        return [(bytes(r[:200]), bytes(r[200:])) for r in rows]


    # ---- results sorted out on the device (efes_objects_results)
    def _results_args(self, expected, compare):
        """(expected, compare) of results() and verify(), checked from the arguments alone: no device is touched."""
        if compare is None:  # the digests the set keeps
            compare = (EFES_HASH_SHA1 if self.has_sha1 else 0) | (EFES_HASH_CRC32 if self.has_crc32 else 0)
        if isinstance(compare, bool) or not isinstance(compare, (int, np.integer)) or compare < 0 or compare & ~(EFES_HASH_SHA1 | EFES_HASH_CRC32):
            raise ValueError(f"DeviceObjects: compare={compare!r} (EFES_HASH_SHA1 | EFES_HASH_CRC32, or 0)")
        if expected is not None:
            if not hasattr(expected, "data_ptr"):
                expected = np.asarray(expected)
            if tuple(expected.shape) != (self.nobjects, 24) or str(expected.dtype) not in ("uint8", "torch.uint8"):
                raise ValueError(f"DeviceObjects: expected is a ({self.nobjects}, 24) uint8 array, laid out like the sums "
                                 f"(got {tuple(expected.shape)} {expected.dtype})")
            if hasattr(expected, "data_ptr") and not expected.is_contiguous():
                raise ValueError("DeviceObjects: expected is a contiguous tensor")
        return expected, int(compare)

    def _results_call(self, expected, compare, records: bool):
        """efes_objects_results on torch's current stream, over buffers the set allocates once and keeps; the record
        array (a device tensor) when asked for.  A host-built set uploads its nobjects + 1 boundaries the first
        time; a set built from a device table uses that table's and copies nothing to the host."""
        torch, device, m = self.torch, self.device, self.nobjects
        d = self.__dict__
        if "_res_first" not in d:
            first = d.get("_table_first")
            if first is None:
                first = torch.from_numpy(np.concatenate((self.first, [self.n])).astype(np.uint32).view(np.int32)).to(device)
            self._res_counts = torch.zeros(4, dtype=torch.int32, device=device)
            self._res_bad = torch.empty(max(m, 1), dtype=torch.int32, device=device)
            self._res_scratch = torch.empty(max(objects_results_scratch(m, self.n), 16), dtype=torch.uint8, device=device)
            self._res_first = first
        if expected is not None and not hasattr(expected, "data_ptr"):
            expected = torch.from_numpy(np.ascontiguousarray(expected)).to(device)
        elif expected is not None and str(expected.device) != str(torch.device(device)):
            expected = expected.to(device)
        if records and "_res_records" not in d:  # kept like the other buffers: it outlives every launch that writes it
            self._res_records = torch.empty(max(m, 1) * OBJECT_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=device)
        rec = self._res_records if records else None
        table = Objects(first=self._res_first.data_ptr(), sums=self.sums.data_ptr(), status=self.status.data_ptr(),
                        nobjects=m, nextents=self.n)
        req = Results(expected=(expected.data_ptr() or None) if expected is not None else None, compare=compare,
                      results=rec.data_ptr() if records else None, bad=self._res_bad.data_ptr(), counts=self._res_counts.data_ptr())
        self._ordered(lambda stream: self.ctx.objects_results(table, req, self._res_scratch.data_ptr(), self._res_scratch.numel(), stream))
        self._res_expected = expected  # alive until the next call
        return rec

    def _results_fetch(self):
        """(counts, bad): the 16 bytes of the counters, then as many words of the list as they say."""
        counts = self._res_counts.cpu().numpy().view(np.uint32).copy()
        nbad = int(counts[1]) + int(counts[2])
        bad = self._res_bad[:nbad].cpu().numpy().view(np.uint32).copy() if nbad else np.zeros(0, np.uint32)
        return counts, bad

    def verify(self, expected, compare=None):
        """(counts, bad): counts[v] = the objects with verdict v (EFES_VERDICT_OK, MISMATCH, FAILED, EMPTY), bad =
        the ascending indices of the objects whose verdict is MISMATCH or FAILED, sorted out on the device by
        efes_objects_results from the sums and statuses the last run left.  expected is a (nobjects, 24) uint8
        array laid out like a sum (the SHA-1 Sum, then the CRC big-endian), host numpy or a device tensor, or
        None: nothing is compared and only failures are bad.  compare = EFES_HASH_SHA1 | EFES_HASH_CRC32 selects
        the bytes compared; the default is the digests the set keeps.  On torch's current stream, behind the run;
        only the 16 bytes of counts and then bad[:counts[1] + counts[2]] are copied to the host."""
        expected, compare = self._results_args(expected, compare)
        self._results_call(expected, compare, records=False)
        return self._results_fetch()

    def results(self, expected=None, compare=None):
        """(records, counts, bad): records is the per-object array of OBJECT_RESULT_DTYPE -- the sum of the object's
        last extent (zeros where it failed or the object has no extents), the status of its first member that is
        not EFES_OK, the verdict --, counts and bad as verify() gives them."""
        expected, compare = self._results_args(expected, compare)
        rec = self._results_call(expected, compare, records=True)
        counts, bad = self._results_fetch()
        return rec.cpu().numpy()[: self.nobjects * OBJECT_RESULT_DTYPE.itemsize].view(OBJECT_RESULT_DTYPE).copy(), counts, bad


class PinnedHostBuffer:
    """Pinned host memory from efes_host_alloc (a socket-buffer pool registered for DMA)."""

    def __init__(self, nbytes: int, ctx: Context | None = None):
        import ctypes

        from ._lib import check, lib

        self.ctx = ctx or default_context()
        p = ctypes.c_void_p()
        check(lib().efes_host_alloc(self.ctx.handle, nbytes, ctypes.byref(p)), "efes_host_alloc")
        self.ptr = p.value
        self.nbytes = nbytes
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * max(nbytes, 1)).from_address(self.ptr))[:nbytes]

    def free(self) -> None:
        from ._lib import lib

        if self.ptr:
            self.array = None
            lib().efes_host_free(self.ctx.handle, self.ptr)
            self.ptr = None

    def __del__(self):  # pragma: no cover - interpreter teardown order
        try:
            self.free()
        except Exception:
            pass


class HostBatch:
    """Jobs whose bytes, states and sums live in HOST memory (efes_hash_host).

    Message j = host bytes [data_ptr + offsets[j], + lengths[j]); each is copied to HBM in
    `segment_bytes` pieces on a copy stream while the previous piece hashes (the per-PATCH
    resume of filereceiver.go:182-226, with the state kept on the device).
    """

    def __init__(self, data_ptr: int, offsets, lengths, *, sha1: bool = True, crc32: bool = True,
                 finalize: bool = True, fresh: bool = True, states: np.ndarray | None = None,
                 crcs: np.ndarray | None = None, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        offsets = np.asarray(offsets, dtype=np.uint64)
        lengths = np.asarray(lengths, dtype=np.uint64)
        n = self.n = int(offsets.size)
        self.states = fresh_states(n) if states is None else np.array(states, dtype=SHA1_STATE_DTYPE)
        self.crcs = np.zeros(n, np.uint32) if crcs is None else np.array(crcs, dtype=np.uint32)
        self.sums = np.zeros((max(n, 1), 24), np.uint8)
        self.status = np.full(max(n, 1), -99, np.int32)
        jobs = np.zeros(n, dtype=JOB_DTYPE)
        jobs["data"] = np.uint64(data_ptr) + offsets
        jobs["length"] = lengths
        idx = np.arange(n, dtype=np.uint64)
        if sha1:
            jobs["sha1"] = np.uint64(self.states.ctypes.data) + idx * np.uint64(SHA1_STATE_DTYPE.itemsize)
        if crc32:
            jobs["crc32"] = np.uint64(self.crcs.ctypes.data) + idx * np.uint64(4)
        if finalize:
            jobs["sum"] = np.uint64(self.sums.ctypes.data) + idx * np.uint64(24)
            jobs["flags"] |= EFES_JOB_FINALIZE
        if fresh:
            jobs["flags"] |= EFES_JOB_INIT
        jobs["status"] = np.uint64(self.status.ctypes.data) + idx * np.uint64(4)
        self.jobs = jobs

    def run(self, segment_bytes: int = 1 << 20):
        """Returns efes_host_stats (seconds, bytes, segments) of the copy+hash pipeline."""
        import ctypes

        from ._lib import HostStats, check, lib

        st = HostStats()
        check(lib().efes_hash_host(self.ctx.handle, self.jobs.ctypes.data, self.n, segment_bytes,
                                   ctypes.byref(st)), "efes_hash_host")
        return st

    def sha1_hex(self) -> list[str]:
        return [bytes(r[:20]).hex() for r in self.sums[: self.n]]

    def crc_sum(self) -> np.ndarray:
        return self.crcs[: self.n]
