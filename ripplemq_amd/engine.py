"""Python handle over the C-ABI engine (numpy in, numpy out).

Thin host glue for tests, tools and bench.py: every call goes straight to
``libripplemq_engine.so``; nothing here computes the data path.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from dataclasses import dataclass

import numpy as np

from . import _abi as A


class EngineError(RuntimeError):
    def __init__(self, status: int, what: str):
        self.status = status
        super().__init__(f"{what}: {A.STATUS_NAMES.get(status, status)}")


def _check(rc: int, what: str) -> int:
    if rc < 0:
        raise EngineError(rc, what)
    return rc


def _ptr(a: np.ndarray | None) -> int | None:
    return None if a is None else a.ctypes.data


_PTRS: dict = {}  # id(array) -> (weak reference, data address): arrays a caller reuses call after call
_PTR_CACHE = os.environ.get("RMQ_PY_PTR_CACHE", "1") != "0"  # (A/B of the cache)


def _budgets(max_bytes, n: int) -> np.ndarray | None:
    """The byte budgets of n fetch requests as rmq_fetch_bytes takes them: an array, or a scalar for
    every request; None: no budgets (plain rmq_fetch)."""
    if max_bytes is None:
        return None
    b = np.broadcast_to(np.asarray(max_bytes, np.uint64), (n,))
    if np.any(b > 0xFFFFFFFF):
        raise ValueError("max_bytes: budgets are 32-bit")
    return np.ascontiguousarray(b, np.uint32)


def _offsets(offsets, n: int) -> np.ndarray | None:
    """The explicit offsets of n fetch requests as rmq_fetch_at takes them: an array, or one value for
    every request; an entry None or RMQ_OFFSET_NONE: that request reads from its committed offset.
    None: no offsets (rmq_fetch / rmq_fetch_bytes)."""
    if offsets is None:
        return None
    if not np.isscalar(offsets) and not isinstance(offsets, np.ndarray):
        offsets = [A.RMQ_OFFSET_NONE if o is None else int(o) for o in offsets]
    return np.ascontiguousarray(np.broadcast_to(np.asarray(offsets, np.uint64), (n,)), np.uint64)


def _host_table(table, n: int, out_cap: int):
    """(rec_row, rec_pos, rec_cap) of a host record table (rmq_fetch_table): True: fresh arrays of the
    size that always suffices, out_cap / 16 + n words; or the caller's (rec_row, rec_pos[, rec_cap])
    uint64 arrays, rec_pos None: the size probe."""
    if table is True:
        cap = int(out_cap) // 16 + n
        return np.zeros(n + 1, np.uint64), np.zeros(max(cap, 1), np.uint64), cap
    row, pos = table[0], table[1]
    return row, pos, int(table[2]) if len(table) > 2 else (0 if pos is None else pos.size)


def _ptr_reused(a: np.ndarray) -> int:
    """_ptr of an array passed again and again (a fetch's request and result rows, views of
    page-locked memory from fetch_rows): numpy's .ctypes.data costs ~1.5 us a call, a checked cache
    entry ~0.5 us."""
    if a.base is None or not _PTR_CACHE:  # (an array owning its data can be resized in place: not cached)
        return a.ctypes.data
    e = _PTRS.get(id(a))
    if e is not None and e[0]() is a:
        return e[1]
    if len(_PTRS) > 256:
        _PTRS.clear()
    p = a.ctypes.data
    try:
        _PTRS[id(a)] = (weakref.ref(a), p)
    except TypeError:  # (an object without weak references: no cache)
        pass
    return p


FETCH_RES_DTYPE = np.dtype([
    ("start_offset", "<u8"), ("out_pos", "<u8"), ("count", "<u4"), ("bytes", "<u4"),
    ("status", "<i4"), ("reserved", "<u4"),
])
LAG_RES_DTYPE = np.dtype([
    ("start_offset", "<u8"), ("records", "<u8"), ("bytes", "<u8"), ("evicted", "<u8"), ("start_pos", "<u8"),
    ("end_pos", "<u8"), ("headroom", "<u8"), ("status", "<i4"), ("reserved", "<u4"),
])
UNPACK_ARGS_DTYPE = np.dtype([
    ("buf", "<u8"), ("buf_bytes", "<u8"), ("rows", "<u8"), ("rec_row", "<u8"), ("rec_pos", "<u8"), ("rec_words", "<u8"),
    ("row_tag", "<u8"), ("rec_first", "<u8"), ("offset", "<u8"), ("len", "<u8"), ("payload_off", "<u8"), ("tag", "<u8"),
    ("rec_cap", "<u8"), ("payload", "<u8"), ("payload_cap", "<u8"), ("n", "<u4"), ("stride", "<u4"), ("mem", "<u4"),
    ("flags", "<u4"),
])
UNPACK_RES_DTYPE = np.dtype([
    ("records", "<u8"), ("payload_bytes", "<u8"), ("mismatched", "<u8"), ("truncated", "<u8"), ("bad_row", "<u8"),
    ("status", "<i4"), ("reserved", "<u4"),
])
SCRUB_RES_DTYPE = np.dtype([
    ("records_ok", "<u8"), ("bytes_ok", "<u8"), ("bad_offset", "<u8"), ("bad_replica", "<u4"),
    ("bad_kind", "<u4"), ("replicas", "<u4"), ("status", "<i4"),
])
REPAIR_RES_DTYPE = np.dtype([
    ("segments_repaired", "<u8"), ("bytes_repaired", "<u8"), ("segments_unrepaired", "<u8"),
    ("bad_offset", "<u8"), ("bad_replica", "<u4"), ("bad_kind", "<u4"), ("replicas", "<u4"), ("status", "<i4"),
])
REINDEX_RES_DTYPE = np.dtype([
    ("entries_live", "<u8"), ("entries_rewritten", "<u8"), ("gaps_unresolved", "<u8"),
    ("bad_offset", "<u8"), ("bad_replica", "<u4"), ("bad_kind", "<u4"), ("replicas", "<u4"), ("status", "<i4"),
])
REPAIR_REMOTE_RES_DTYPE = np.dtype([
    ("segments_repaired", "<u8"), ("bytes_repaired", "<u8"), ("segments_fetched", "<u8"), ("bytes_fetched", "<u8"),
    ("segments_unrepaired", "<u8"), ("bad_offset", "<u8"), ("bad_replica", "<u4"), ("bad_kind", "<u4"),
    ("replicas", "<u4"), ("status", "<i4"),
])
RESTORE_ITEM_DTYPE = np.dtype([
    ("pidx", "<u4"), ("flags", "<u4"), ("first_offset", "<u8"), ("first_pos", "<u8"), ("count", "<u8"),
    ("bytes", "<u8"), ("buf_pos", "<u8"), ("table_start", "<u8"), ("commit", "<u8"),
])
RESTORE_RES_DTYPE = np.dtype([
    ("records", "<u8"), ("bytes", "<u8"), ("bad_offset", "<u8"), ("bad_kind", "<u4"), ("status", "<i4"),
])
STATE_FIELDS = ("log_end_offset", "log_end_pos", "log_start_offset", "log_start_pos", "commit",
                "high_watermark", "term", "term_start", "leader_commit", "last_log_term", "voted_term",
                "voted_for", "led", "heard_round")


@dataclass
class EngineConfig:
    num_partitions: int
    replication_factor: int = 3
    segment_bytes: int = 1 << 20
    index_interval: int = 1024
    max_consumers: int = 8
    max_batch_records: int = 65536
    pipeline_depth: int = 2          # batches per pipeline launch group (1..8)
    max_batch_bytes: int = 64 << 20
    device: int = 0
    rank: int = 0
    pool_bytes: int = 0              # ring bytes per replica shared by all partitions (0: P * segment)

    def to_c(self) -> A.RmqConfig:
        c = A.RmqConfig()
        for f, _ in A.RmqConfig._fields_:
            setattr(c, f, getattr(self, f))
        return c


# numpy mirror of rmq_partition_state (bulk read-back)
STATE_DTYPE = np.dtype({"names": [f for f, _ in A.RmqPartitionState._fields_],
                        "formats": ["<u8"] * 8 + [("<u8", A.RMQ_MAX_RF), ("<u4", A.RMQ_MAX_RF), "<u4", "<u4",
                                                  "<u8", "<u8", "<u8", "<u8", "<u4", "<u4", "<u8"],
                        "offsets": [getattr(A.RmqPartitionState, f).offset for f, _ in A.RmqPartitionState._fields_],
                        "itemsize": C.sizeof(A.RmqPartitionState)})


def state_to_dict(s: A.RmqPartitionState, rf: int) -> dict:
    d = {f: int(getattr(s, f)) for f in STATE_FIELDS}
    d["match"] = [int(s.match[r]) for r in range(rf)]
    d["replica_rank"] = [int(s.replica_rank[r]) for r in range(rf)]
    d["leader_slot"] = int(s.leader_slot)
    d["is_leader"] = int(s.is_leader)
    d["segment_bytes"] = int(s.segment_bytes)
    return d


class FetchTicket:
    """An rmq_fetch_async in flight: its ticket and the arrays the engine writes into."""
    __slots__ = ("ticket", "req", "res", "out", "table")

    def __init__(self, ticket: int, req: np.ndarray, res: np.ndarray, out: np.ndarray | None, table=None):
        self.ticket, self.req, self.res, self.out, self.table = ticket, req, res, out, table


class Engine:
    """One engine = one HIP device, P partitions, RF co-located or placed replicas."""

    def __init__(self, cfg: EngineConfig, lib_path: str | None = None):
        self.lib = A.load(lib_path) if lib_path else A.load()
        self.cfg = cfg
        h = C.c_void_p()
        c = cfg.to_c()
        _check(self.lib.rmq_create(C.byref(c), C.byref(h)), "rmq_create")
        self.h = h
        self._keep: dict[int, tuple] = {}
        self._pinned: dict[int, np.ndarray] = {}  # rmq_host_alloc buffers by address
        # fetches in flight by ticket: the engine holds raw pointers to their arrays (results, output,
        # page-locked requests) until rmq_fetch_poll answers them or the engine is destroyed
        self._fetching: dict[int, "FetchTicket"] = {}
        # append_device reuses one argument block: a producer loop calls it once per batch
        self._dbatch = A.RmqBatch(0, A.RMQ_MEM_DEVICE)
        self._dticket = C.c_uint64()
        self._dargs = (C.byref(self._dbatch), C.byref(self._dticket))
        self.transport = False  # a replication transport is attached (rounds are collective)
        self.last_offset_ticket = 0
        self.last_scrub_rc = A.RMQ_OK

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.rmq_destroy(self.h)
            self.h = None
            self._keep.clear()
            self._fetching.clear()  # (rmq_destroy waited for every fetch)
            for p in list(self._pinned):  # after the engine: no DMA reads them any more
                self.lib.rmq_host_free(None, C.c_void_p(p))
            self._pinned.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- control
    def set_replicas(self, pidx: int, ranks, leader_slot: int) -> None:
        r = (C.c_uint32 * len(ranks))(*ranks)
        _check(self.lib.rmq_set_replicas(self.h, pidx, r, len(ranks), leader_slot), "rmq_set_replicas")

    def set_placement(self, pidx, keys, ranks, leader_slot) -> None:
        """rmq_set_placement: ranks is [n][RF]; keys may be None (unchanged)."""
        pidx = np.ascontiguousarray(pidx, np.uint32)
        ranks = np.ascontiguousarray(ranks, np.uint32).reshape(len(pidx), self.cfg.replication_factor)
        leader_slot = np.ascontiguousarray(leader_slot, np.uint32)
        keys = None if keys is None else np.ascontiguousarray(keys, np.uint64)
        _check(self.lib.rmq_set_placement(self.h, len(pidx), _ptr(pidx), _ptr(keys), _ptr(ranks), _ptr(leader_slot)),
               "rmq_set_placement")

    def attach_local(self, hub: "LocalHub") -> None:
        _check(self.lib.rmq_attach_local(self.h, hub.h), "rmq_attach_local")
        self.transport = True

    def attach_rccl(self, comm_id: bytes, world: int) -> None:
        buf = (C.c_uint8 * 128).from_buffer_copy(comm_id)
        _check(self.lib.rmq_attach_rccl(self.h, buf, world), "rmq_attach_rccl")
        self.transport = True

    def replication_stats(self) -> dict:
        st = A.RmqReplStats()
        _check(self.lib.rmq_replication_stats(self.h, C.byref(st)), "rmq_replication_stats")
        return {f: int(getattr(st, f)) for f, _ in A.RmqReplStats._fields_}

    def read_outbox(self, dst: int) -> np.ndarray:
        n = C.c_uint64()
        _check(self.lib.rmq_read_outbox(self.h, dst, None, 0, C.byref(n)), "rmq_read_outbox")
        out = np.zeros(max(int(n.value), 1), np.uint8)
        _check(self.lib.rmq_read_outbox(self.h, dst, _ptr(out), out.size, C.byref(n)), "rmq_read_outbox")
        return out[:int(n.value)]

    def fault_drop_rounds(self, n: int = 1) -> None:
        """Tests: the next n rounds this engine leads carry no records (rmq_fault_drop_rounds)."""
        _check(self.lib.rmq_fault_drop_rounds(self.h, n), "rmq_fault_drop_rounds")

    def fault_isolate(self, dst: int, n: int = 1) -> None:
        """Tests: the next n rounds this engine sends to dst are lost (rmq_fault_isolate)."""
        _check(self.lib.rmq_fault_isolate(self.h, dst, n), "rmq_fault_isolate")

    def fault_corrupt(self, dst: int, at: int) -> None:
        """Tests: the next round sent to dst has one byte flipped (rmq_fault_corrupt)."""
        _check(self.lib.rmq_fault_corrupt(self.h, dst, at), "rmq_fault_corrupt")

    def fault_cut(self, dst: int, n: int = 1) -> None:
        """Tests: as fault_isolate, and the next drain's commit notices to dst are lost (rmq_fault_cut)."""
        _check(self.lib.rmq_fault_cut(self.h, dst, n), "rmq_fault_cut")

    def become_leader(self, pidx: int, term: int) -> None:
        _check(self.lib.rmq_become_leader(self.h, pidx, term), "rmq_become_leader")

    def vote(self, pidx: int, term: int, candidate: int, cand_last_log_term: int, cand_log_end: int) -> bool:
        """Raft RequestVote on this replica (rmq_vote): True if the vote was granted."""
        g = C.c_uint32(0)
        _check(self.lib.rmq_vote(self.h, pidx, term, candidate, cand_last_log_term, cand_log_end, C.byref(g)),
               "rmq_vote")
        return bool(g.value)

    def set_replica_cursor(self, pidx, offset) -> None:
        """Where RMQ_FETCH_REPLICA reads of these partitions start (rmq_set_replica_cursor)."""
        pidx = np.ascontiguousarray(pidx, np.uint32)
        offset = np.ascontiguousarray(offset, np.uint64)
        _check(self.lib.rmq_set_replica_cursor(self.h, len(pidx), _ptr(pidx), _ptr(offset)), "rmq_set_replica_cursor")

    def set_vote(self, pidx: int, term: int, voted_for: int) -> None:
        """Replay of a persisted vote (rmq_set_vote)."""
        _check(self.lib.rmq_set_vote(self.h, pidx, term, voted_for), "rmq_set_vote")

    def leader_silent(self, silent_rounds: int, timeout_ms: int = 0) -> np.ndarray:
        """Followed partitions whose leader has been silent (rmq_leader_silent)."""
        n = C.c_uint32(0)
        _check(self.lib.rmq_leader_silent(self.h, silent_rounds, timeout_ms, None, 0, C.byref(n)), "rmq_leader_silent")
        out = np.zeros(max(n.value, 1), np.uint32)
        _check(self.lib.rmq_leader_silent(self.h, silent_rounds, timeout_ms, _ptr(out), n.value, C.byref(n)),
               "rmq_leader_silent")
        return out[:n.value]

    # ---- append
    def append_async(self, pidx: np.ndarray, lens: np.ndarray, payload: np.ndarray,
                     payload_off: np.ndarray | None = None) -> tuple[int, np.ndarray]:
        pidx = np.ascontiguousarray(pidx, dtype=np.uint32)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        payload = np.ascontiguousarray(payload, dtype=np.uint8)
        if payload_off is not None:
            payload_off = np.ascontiguousarray(payload_off, dtype=np.uint64)
        out = np.empty(len(pidx), dtype=np.uint64)
        b = A.RmqBatch(len(pidx), A.RMQ_MEM_HOST, _ptr(pidx), _ptr(lens), _ptr(payload_off),
                       _ptr(payload) if payload.size else None, payload.size)
        t = C.c_uint64()
        _check(self.lib.rmq_append(self.h, C.byref(b), _ptr(out), C.byref(t)), "rmq_append")
        self._keep[t.value] = (pidx, lens, payload, payload_off, out)
        return t.value, out

    # ---- page-locked host batches (RMQ_MEM_PINNED)
    def host_empty(self, count: int, dtype) -> np.ndarray:
        """A numpy array in page-locked host memory (rmq_host_alloc), freed with the engine or by
        host_release. Batches whose arrays all come from here go to the device by DMA alone."""
        dtype = np.dtype(dtype)
        nbytes = max(int(count) * dtype.itemsize, 16)
        p = C.c_void_p()
        _check(self.lib.rmq_host_alloc(self.h, nbytes, C.byref(p)), "rmq_host_alloc")
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        arr = np.frombuffer(buf, np.uint8, nbytes)[:int(count) * dtype.itemsize].view(dtype)
        self._pinned[p.value] = arr
        return arr

    def host_release(self, arr: np.ndarray) -> None:
        p = arr.__array_interface__["data"][0]
        if self._pinned.pop(p, None) is not None:
            _check(self.lib.rmq_host_free(self.h, C.c_void_p(p)), "rmq_host_free")

    def host_register(self, arr: np.ndarray) -> None:
        """Page-lock a caller's contiguous array in place (rmq_host_register), so it can serve as
        pinned batch arrays or pinned fetch rows; undone by host_unregister before it is freed."""
        if not arr.flags["C_CONTIGUOUS"] or arr.nbytes == 0:
            raise ValueError("host_register needs a non-empty contiguous array")
        _check(self.lib.rmq_host_register(self.h, C.c_void_p(arr.__array_interface__["data"][0]), arr.nbytes),
               "rmq_host_register")

    def host_unregister(self, arr: np.ndarray) -> None:
        _check(self.lib.rmq_host_unregister(self.h, C.c_void_p(arr.__array_interface__["data"][0])),
               "rmq_host_unregister")

    def append_pinned_async(self, pidx: np.ndarray, lens: np.ndarray, payload: np.ndarray, out: np.ndarray,
                            payload_off: np.ndarray | None = None, payload_bytes: int | None = None) -> int:
        """rmq_append of a batch whose arrays (and `out`, uint64[n]) are page-locked (host_empty):
        one DMA per section, no host copy; the arrays must stay unchanged until the ticket
        completes. Payload ranges are checked on the device (rejected_invalid), like device
        batches."""
        n = len(pidx)
        nb = payload.size if payload_bytes is None else int(payload_bytes)
        b = A.RmqBatch(n, A.RMQ_MEM_PINNED, _ptr(pidx), _ptr(lens), _ptr(payload_off),
                       _ptr(payload) if nb else None, nb)
        t = C.c_uint64()
        _check(self.lib.rmq_append(self.h, C.byref(b), _ptr(out), C.byref(t)), "rmq_append")
        return t.value

    def append_device(self, n: int, d_pidx: int, d_len: int, d_payload: int, payload_bytes: int,
                      d_out: int, d_payload_off: int | None = None) -> int:
        b = self._dbatch
        b.n, b.pidx, b.len, b.payload_off, b.payload, b.payload_bytes = (
            n, d_pidx, d_len, d_payload_off, d_payload, payload_bytes)
        rc = self.lib.rmq_append(self.h, self._dargs[0], d_out, self._dargs[1])
        if rc < 0:
            raise EngineError(rc, "rmq_append")
        return self._dticket.value

    def poll(self, ticket: int, want_commit: bool = False):
        P = self.cfg.num_partitions
        commit = np.empty(P, np.uint64) if want_commit else None
        hw = np.empty(P, np.uint64) if want_commit else None
        rc = _check(self.lib.rmq_poll_commit(self.h, ticket, _ptr(commit), _ptr(hw)), "rmq_poll_commit")
        if rc == A.RMQ_PENDING:
            return None
        self._keep.pop(ticket, None)
        return (commit, hw) if want_commit else True

    def wait(self, ticket: int) -> dict | None:
        """Stats of a completed ticket, or None while it is pending: with a replication transport a
        ticket is applied only by an rmq_sync on every rank (the caller's arrays stay referenced
        until then; their out offsets are not written yet)."""
        st = A.RmqAppendStats()
        rc = _check(self.lib.rmq_ticket_stats(self.h, ticket, C.byref(st)), "rmq_ticket_stats")
        if rc == A.RMQ_PENDING:
            return None
        self._keep.pop(ticket, None)
        return {f: int(getattr(st, f)) for f, _ in A.RmqAppendStats._fields_}

    def append(self, pidx, lens, payload, payload_off=None) -> tuple[np.ndarray, dict]:
        """Synchronous append: offsets and stats of the batch. With a replication transport the
        batch is applied only by a collective rmq_sync, so this raises RMQ_PENDING (keep the
        ticket: append_async + sync + wait). The check comes before anything is queued, so a caller
        that retries after the error never appends the records twice."""
        if self.transport:
            raise EngineError(A.RMQ_PENDING, "rmq_append (transport attached: use append_async, then rmq_sync "
                                             "on every rank applies it)")
        t, out = self.append_async(pidx, lens, payload, payload_off)
        stats = self.wait(t)
        if stats is None:
            raise EngineError(A.RMQ_PENDING, "rmq_append (transport attached: rmq_sync on every rank applies it)")
        return out, stats

    def commit_snapshot(self) -> np.ndarray:
        """Commit index of every partition after everything submitted so far."""
        P = self.cfg.num_partitions
        commit = np.empty(P, np.uint64)
        _check(self.lib.rmq_poll_commit(self.h, 0, _ptr(commit), None), "rmq_poll_commit")
        return commit

    def sync(self) -> None:
        _check(self.lib.rmq_sync(self.h), "rmq_sync")
        self._keep.clear()  # every ticket is complete: its out offsets are in the caller's arrays

    def ack(self, pidx, slot, match) -> None:
        pidx = np.ascontiguousarray(pidx, np.uint32)
        slot = np.ascontiguousarray(slot, np.uint32)
        match = np.ascontiguousarray(match, np.uint64)
        _check(self.lib.rmq_ack(self.h, _ptr(pidx), _ptr(slot), _ptr(match), len(pidx)), "rmq_ack")

    def commit_consumer_offset(self, pidx, consumer, offset) -> tuple[int, np.ndarray]:
        """rmq_commit_consumer_offset: (rc, per-item status); the call's ticket (0 if no item was
        accepted) is in self.last_offset_ticket, for poll_offsets."""
        pidx = np.ascontiguousarray(pidx, np.uint32)
        consumer = np.ascontiguousarray(consumer, np.uint32)
        offset = np.ascontiguousarray(offset, np.uint64)
        status = np.zeros(len(pidx), np.int32)
        t = C.c_uint64()
        rc = self.lib.rmq_commit_consumer_offset(self.h, _ptr(pidx), _ptr(consumer), _ptr(offset),
                                                 len(pidx), _ptr(status), C.byref(t))
        if rc in (A.RMQ_EDEVICE, A.RMQ_ENOMEM):
            raise EngineError(rc, "rmq_commit_consumer_offset")
        self.last_offset_ticket = int(t.value)
        return rc, status

    def poll_offsets(self, ticket: int) -> int:
        """rmq_poll_commit of a consumer-offset ticket: RMQ_OK (the rows are on a quorum),
        RMQ_PENDING, or RMQ_ENOTLEADER (leadership moved first: the commit may be lost)."""
        rc = self.lib.rmq_poll_commit(self.h, ticket, None, None)
        if rc not in (A.RMQ_OK, A.RMQ_PENDING, A.RMQ_ENOTLEADER):
            raise EngineError(rc, "rmq_poll_commit (offsets)")
        return rc

    def _fetch_call(self, asyn: bool, req, n: int, mem: int, out, out_cap: int, res, last, at=None, bud=None, tab=None):
        """One fetch through the narrowest C entry point that takes it, so that all ten stay in use:
        rmq_fetch_table with a table (rec_row, rec_pos, rec_cap), else rmq_fetch_at with offsets, else
        rmq_fetch_bytes with budgets, else rmq_fetch; asyn: its _async twin. Every array is an address
        or None; last: the bytes_used / ticket word. Returns (rc, the entry point's name)."""
        if tab is not None:
            name, a = "rmq_fetch_table", (req, at, bud, n, mem, out, out_cap, res, *tab, last)
        elif at is not None:
            name, a = "rmq_fetch_at", (req, at, bud, n, mem, out, out_cap, res, last)
        elif bud is not None:
            name, a = "rmq_fetch_bytes", (req, bud, n, mem, out, out_cap, res, last)
        else:
            name, a = "rmq_fetch", (req, n, mem, out, out_cap, res, last)
        if asyn:
            name += "_async"
        return getattr(self.lib, name)(self.h, *a), name

    @staticmethod
    def _fetch_rows(n: int, req, res, cols, flags: int = 0, fresh_flags: int = 0):
        """The request and result rows of a call: the caller's arrays, or fresh zeroed ones (their
        flags column then fresh_flags). cols = (pidx, consumer, max_records): None leaves that column
        of req as it is; flags are ORed into every request."""
        if req is None:
            req = np.zeros((n, 4), np.uint32)
            req[:, 3] = fresh_flags
        if flags:
            req[:, 3] |= flags
        for col, v in enumerate(cols):
            if v is not None:
                req[:, col] = v
        return req, np.zeros(n, FETCH_RES_DTYPE) if res is None else res

    def fetch(self, pidx, consumer, max_records, out_cap: int | None = None, commit: bool = False,
              out: np.ndarray | None = None, replica: bool = False, verify: bool = False, max_bytes=None,
              offsets=None, fill: bool = False, table=None):
        """rmq_fetch into a host array (sized by a first call when out_cap is None, or the caller's
        uint8 `out`, e.g. page-locked from host_empty: one call, RMQ_ENOSPC if it is too small);
        commit: RMQ_FETCH_COMMIT on every request (the size query commits nothing); replica:
        RMQ_FETCH_REPLICA (this engine's own replica from its replica cursor, leader or follower);
        verify: RMQ_FETCH_VERIFY (a slice with a record that fails its checks comes back
        RMQ_ECORRUPT with count 0). max_bytes: a byte budget per request (an array, or one value
        for all; 0: none): rmq_fetch_bytes, FORMAT.md §7. offsets: an explicit start offset per
        request (an array, or one value for all; None or RMQ_OFFSET_NONE entries: the committed
        offset): rmq_fetch_at, FORMAT.md §7; the size query reads at the same offsets. fill:
        RMQ_FETCH_FILL (FORMAT.md §7 "Filling a bounded output": requests are served in order until
        the output is full, the rest come back RMQ_PENDING); needs out_cap or out (no sizing call).
        table: a record table with the fetch (rmq_fetch_table, FORMAT.md §7 "Record table"): True,
        or the caller's (rec_row, rec_pos[, rec_cap]) uint64 arrays (rec_pos None: the size probe);
        the call then returns (rc, res, out, bytes_used, rec_row, rec_pos), RMQ_ENOSPC also when
        rec_row[n] > rec_cap; table_records splits the output with it."""
        n = len(pidx)
        if fill and out is None and out_cap is None:
            raise ValueError("fill needs out_cap or out: a filling fetch has no sizing call")
        bud = _budgets(max_bytes, n)
        at = _offsets(offsets, n)
        req, res = self._fetch_rows(n, None, None, (pidx, consumer, max_records),
                                    (A.RMQ_FETCH_REPLICA if replica else 0) | (A.RMQ_FETCH_VERIFY if verify else 0))
        used = C.c_uint64()

        def call(mem, out, cap, tab=None):
            rc, _ = self._fetch_call(False, _ptr(req), n, mem, _ptr(out), cap, _ptr(res), C.byref(used), _ptr(at),
                                     _ptr(bud), tab and (_ptr(tab[0]), _ptr(tab[1]), tab[2]))
            if rc not in (A.RMQ_OK, A.RMQ_ENOSPC):
                raise EngineError(rc, "rmq_fetch")
            return rc

        ret = out  # (the caller's array as it came; a fresh one cut to out_cap)
        if out is not None:
            out_cap = out.size
        elif out_cap is None:  # the size query: no flags of the call, no table, nothing committed
            call(A.RMQ_MEM_HOST, None, 0)
            out_cap = int(used.value)
        if out is None:
            out = np.zeros(max(out_cap, 1), np.uint8)
            ret = out[:out_cap]
        if commit:
            req[:, 3] |= A.RMQ_FETCH_COMMIT
        # (the table's arrays once the output's size is known)
        tab = _host_table(table, n, out_cap) if table else None
        rc = call(A.RMQ_MEM_HOST | (A.RMQ_FETCH_FILL if fill else 0), out, out_cap, tab)
        return (rc, res, ret, int(used.value)) + (tuple(tab[:2]) if table else ())

    def fetch_device(self, pidx, consumer, max_records, d_out: int, out_cap: int, commit: bool = False,
                     req: np.ndarray | None = None, res: np.ndarray | None = None, pinned_rows: bool = False,
                     d_rows: tuple | None = None, verify: bool = False, max_bytes=None, offsets=None,
                     fill: bool = False, table=None):
        """rmq_fetch into a device buffer (16-byte aligned); returns (rc, res, bytes_used). req / res:
        the caller's arrays (pidx / consumer / max_records None leave req's columns as they are);
        pinned_rows: page-locked ones (fetch_rows), read and written by the kernels in place
        (RMQ_FETCH_PINNED_ROWS). d_rows = (n, device request rows, device result rows): rows in
        device memory (RMQ_FETCH_DEVICE_ROWS, flags ignored), with an optional fourth element, the
        device array of the requests' byte budgets (uint32[n]); res is then None. verify:
        RMQ_FETCH_VERIFY on every request (host rows only). max_bytes: byte budgets of host rows, as
        for fetch. offsets: explicit offsets of host rows, as for fetch (rmq_fetch_at); with d_rows
        the address of a device array (uint64[n], 8-byte aligned). fill: RMQ_FETCH_FILL, as for fetch
        (every kind of rows). table = (d_rec_row, d_rec_pos, rec_cap): a record table in device memory
        (rmq_fetch_table; uint64[n + 1] and uint64[rec_cap], 8-byte aligned; d_rec_pos 0 / None with
        rec_cap 0: the size probe), with any kind of rows; the two addresses are then returned too."""
        tb = None if table is None else (C.c_void_p(table[0]), C.c_void_p(table[1] or None), int(table[2]))
        ret = () if table is None else (table[0], table[1])
        used = C.c_uint64()
        mem = A.RMQ_MEM_DEVICE | (A.RMQ_FETCH_FILL if fill else 0)
        if d_rows is not None:
            if max_bytes is not None:
                raise ValueError("device rows take their budgets as d_rows' fourth element")
            n, res, mem = d_rows[0], None, mem | A.RMQ_FETCH_DEVICE_ROWS
            p_req, p_res = C.c_void_p(d_rows[1]), C.c_void_p(d_rows[2])
            p_at = None if offsets is None else C.c_void_p(int(offsets))
            p_bud = C.c_void_p(d_rows[3]) if len(d_rows) > 3 and d_rows[3] else None
        else:
            n = len(pidx) if pidx is not None else len(req)
            req, res = self._fetch_rows(n, req, res, (pidx, consumer, max_records), A.RMQ_FETCH_VERIFY if verify else 0,
                                        A.RMQ_FETCH_COMMIT if commit else 0)
            if pinned_rows:
                mem |= A.RMQ_FETCH_PINNED_ROWS
            bud, at = _budgets(max_bytes, n), _offsets(offsets, n)  # (alive until the call returns)
            p_req, p_res, p_at, p_bud = _ptr_reused(req), _ptr_reused(res), _ptr(at), _ptr(bud)
        rc, _ = self._fetch_call(False, p_req, n, mem, d_out, out_cap, p_res, C.byref(used), p_at, p_bud, tb)
        if rc not in (A.RMQ_OK, A.RMQ_ENOSPC):
            raise EngineError(rc, "rmq_fetch")
        return (rc, res, int(used.value)) + ret

    def fetch_async(self, pidx, consumer, max_records, d_out: int | None = None, out_cap: int = 0,
                    out: np.ndarray | None = None, req: np.ndarray | None = None,
                    res: np.ndarray | None = None, pinned_rows: bool = False,
                    verify: bool = False, max_bytes=None, offsets=None, fill: bool = False,
                    table=None) -> "FetchTicket":
        """rmq_fetch_async into a device buffer (d_out, 16-byte aligned) or a host array (out): the
        call returns at once; fetch_poll(ticket) gives (rc, res, bytes_used) once it completes. The
        handle keeps the request, result and output arrays alive until then. req ([n, 4] uint32)
        and res (FETCH_RES_DTYPE[n]) may be a caller's arrays reused from call to call; with req
        given, pidx / consumer / max_records None leave those columns as they are (column 3: the
        requests' flags, RMQ_FETCH_COMMIT). pinned_rows: req and res are page-locked (fetch_rows)
        and the kernels read and write them in place (RMQ_FETCH_PINNED_ROWS); req then stays
        unchanged until the ticket completes. verify: RMQ_FETCH_VERIFY ORed into every request.
        max_bytes: byte budgets, as for fetch (rmq_fetch_bytes_async; read before the call returns).
        offsets: explicit offsets, as for fetch (rmq_fetch_at_async; read before the call returns).
        fill: RMQ_FETCH_FILL, as for fetch. table: a record table (rmq_fetch_table_async): with a
        host output as for fetch (True, or the caller's arrays), with d_out as for fetch_device
        (device addresses); fetch_poll then returns (rc, res, bytes_used, rec_row, rec_pos)."""
        n = len(pidx) if pidx is not None else len(req)
        if pinned_rows and (req is None or res is None):
            raise ValueError("pinned_rows needs the caller's page-locked req and res (fetch_rows)")
        req, res = self._fetch_rows(n, req, res, (pidx, consumer, max_records), A.RMQ_FETCH_VERIFY if verify else 0)
        if d_out is not None:
            mem, ptr = A.RMQ_MEM_DEVICE, C.c_void_p(d_out)
        else:
            out_cap = 0 if out is None else min(int(out_cap) or out.size, out.size)
            mem, ptr = A.RMQ_MEM_HOST, (_ptr(out) if out is not None else None)
        if pinned_rows:
            mem |= A.RMQ_FETCH_PINNED_ROWS
        if fill:
            mem |= A.RMQ_FETCH_FILL
        t = C.c_uint64()
        bud = _budgets(max_bytes, n)
        at = _offsets(offsets, n)
        tb = None
        if table is not None and table is not False:
            if d_out is not None:
                tb = (C.c_void_p(table[0]), C.c_void_p(table[1] or None), int(table[2]))
                table = (table[0], table[1])
            else:
                row, pos, cap = _host_table(table, n, out_cap)
                tb, table = (_ptr(row), _ptr(pos), cap), (row, pos)
        _check(*self._fetch_call(True, _ptr_reused(req), n, mem, ptr, out_cap, _ptr_reused(res), C.byref(t), _ptr(at),
                                 _ptr(bud), tb))
        tk = FetchTicket(t.value, req, res, out, table or None)
        self._fetching[t.value] = tk
        return tk

    def fetch_rows(self, n: int):
        """A page-locked request array ([n, 4] uint32, zeroed) and result array (FETCH_RES_DTYPE[n])
        for fetch_async(..., pinned_rows=True); freed with the engine or by host_release."""
        req = self.host_empty(4 * n, np.uint32).reshape(n, 4)
        req[:] = 0
        return req, self.host_empty(n, FETCH_RES_DTYPE)

    def fetch_poll(self, tk: "FetchTicket", wait: bool = False):
        """(rc, res, bytes_used) of an rmq_fetch_async ticket, or None while it runs; a ticket with a
        record table adds (rec_row, rec_pos)."""
        used = C.c_uint64()
        rc = self.lib.rmq_fetch_poll(self.h, tk.ticket, 1 if wait else 0, C.byref(used))
        if rc == A.RMQ_PENDING:
            return None
        self._fetching.pop(tk.ticket, None)
        if rc not in (A.RMQ_OK, A.RMQ_ENOSPC):
            raise EngineError(rc, "rmq_fetch_poll")
        return (rc, tk.res, int(used.value)) + (tuple(tk.table) if tk.table else ())

    def lag(self, pidx, consumer, offsets=None, replica: bool = False, flags: int = 0) -> np.ndarray:
        """rmq_lag with host rows (FORMAT.md §7 "Lag"): per (pidx[r], consumer[r]) the records and
        bytes between the reader and the high watermark and the partition's retention headroom, as
        LAG_RES_DTYPE rows. offsets: explicit offsets as for fetch (an array, or one value for all;
        None or RMQ_OFFSET_NONE entries: the committed offset, or the replica cursor); replica:
        RMQ_FETCH_REPLICA on every row; flags: further flag bits for every row (RMQ_FETCH_COMMIT
        and RMQ_FETCH_VERIFY do nothing, any other fails the call). Writes nothing of the engine."""
        n = len(pidx)
        req = np.zeros((n, 4), np.uint32)
        req[:, 0], req[:, 1] = pidx, consumer
        req[:, 3] = (A.RMQ_FETCH_REPLICA if replica else 0) | flags
        at = _offsets(offsets, n)
        res = np.zeros(n, LAG_RES_DTYPE)
        _check(self.lib.rmq_lag(self.h, _ptr(req), _ptr(at), n, A.RMQ_MEM_HOST, _ptr(res)), "rmq_lag")
        return res

    def lag_device(self, d_req: int, d_offsets: int | None, n: int, d_res: int) -> None:
        """rmq_lag with rows in device memory, used in place: d_req ([n, 4] uint32) and d_res
        (LAG_RES_DTYPE[n]) 16-byte aligned, d_offsets (uint64[n], 8-byte aligned) or None / 0."""
        _check(self.lib.rmq_lag(self.h, C.c_void_p(d_req), C.c_void_p(d_offsets or None), n, A.RMQ_MEM_DEVICE,
                                C.c_void_p(d_res)), "rmq_lag")

    def unpack_device(self, *, buf: int, buf_bytes: int, rows, n: int, rec_row: int, rec_pos: int, rec_words: int,
                      rec_first: int, len: int = 0, payload_off: int = 0, offset: int = 0, tag: int = 0,  # noqa: A002
                      row_tag: int = 0, rec_cap: int = 0, payload: int = 0, payload_cap: int = 0, stride: int = 0,
                      flags: int = 0) -> dict:
        """rmq_unpack over device addresses (FORMAT.md §7 "Record columns"): the answer of a table
        fetch into a device buffer as columns. Every array is a device address (0 / None: null) but
        rows: the fetch's result rows as a FETCH_RES_DTYPE array (host rows), or the address of
        device rows (RMQ_FETCH_DEVICE_ROWS). payload 0: view mode; stride > 0: strided; else packed.
        Returns the rmq_unpack_res as a dict (status RMQ_OK or RMQ_ENOSPC); raises on anything else,
        the error's `res` attribute holding the dict."""
        mem = A.RMQ_MEM_DEVICE
        if isinstance(rows, np.ndarray):
            rows = np.ascontiguousarray(rows)
            p_rows = _ptr(rows)
        else:
            p_rows, mem = rows or None, mem | A.RMQ_FETCH_DEVICE_ROWS
        a = A.RmqUnpackArgs(buf or None, buf_bytes, p_rows, rec_row or None, rec_pos or None, rec_words,
                            row_tag or None, rec_first or None, offset or None, len or None, payload_off or None,
                            tag or None, rec_cap, payload or None, payload_cap, n, stride, mem, flags)
        out = A.RmqUnpackRes()
        rc = self.lib.rmq_unpack(self.h, C.byref(a), C.byref(out))
        d = {f: int(getattr(out, f)) for f, _ in A.RmqUnpackRes._fields_}
        if rc not in (A.RMQ_OK, A.RMQ_ENOSPC):
            err = EngineError(rc, "rmq_unpack")
            err.res = d
            raise err
        return d

    def fetch_columns(self, pidx, consumer, max_records, *, mode="packed", row_tag=None, out_cap: int | None = None,
                      device_rows: bool = False, keep_device: bool = False, **fetch_kw):
        """A fetch answered as columns (rmq_fetch_table into a device buffer, then rmq_unpack; FORMAT.md
        §7 "Record columns"): (res, columns, payload). res: the fetch's result rows; columns: a dict
        of numpy arrays, rec_first (uint64[n + 1]) and per record offset, len, payload_off, tag, plus
        the rmq_unpack_res words under "unpack"; payload: mode "packed": the payloads back to back
        (record j is payload[payload_off[j]:payload_off[j] + len[j]]); mode "view": the fetch's own
        output, payload_off pointing into it; mode an int stride: an [R, stride] array. row_tag:
        uint32[n], the tag of each row's records (default: the row's index). out_cap: the bytes of
        the device output (default: sized by a query; required with fill). device_rows: the unpack
        reads the result rows from device memory. keep_device: the device arrays stay allocated and
        columns["device"] names them (buf, buf_bytes, offset, len, payload_off, tag, payload, and
        "held": every address to device_free), e.g. to append the columns as they lie. fetch_kw: commit, verify, max_bytes, offsets, fill,
        as for fetch_device."""
        n = len(pidx)
        stride = 0 if isinstance(mode, str) else int(mode)
        if (isinstance(mode, str) and mode not in ("packed", "view")) or (not isinstance(mode, str) and stride <= 0):
            raise ValueError(f"mode: 'packed', 'view' or a positive stride, not {mode!r}")
        if out_cap is None:
            if fetch_kw.get("fill"):
                raise ValueError("fill needs out_cap: a filling fetch has no sizing call")
            q = {k: fetch_kw[k] for k in ("verify", "max_bytes", "offsets") if k in fetch_kw}
            out_cap = self.fetch(pidx, consumer, max_records, out_cap=0, **q)[3]
        out_cap = (int(out_cap) + 15) & ~15
        words = out_cap // 16 + n
        held: list[int] = []

        def dev(nbytes, src=None):
            p = self.device_alloc(max(int(nbytes), 16))
            held.append(p)
            if src is not None:
                self.h2d(p, src)
            return p

        def back(p, count, dtype):
            a = np.empty(count, dtype)
            if count:
                self.d2h(a, p)
            return a

        try:
            d_out, d_row, d_pos, d_first = dev(out_cap), dev(8 * (n + 1)), dev(8 * words), dev(8 * (n + 1))
            rc, res, used = self.fetch_device(pidx, consumer, max_records, d_out, out_cap,
                                              table=(d_row, d_pos, words), **fetch_kw)[:3]
            if rc != A.RMQ_OK:
                raise EngineError(rc, "rmq_fetch_table (fetch_columns)")
            rows = dev(res.nbytes, res) if device_rows else res
            d_tag_in = 0 if row_tag is None else dev(4 * n, np.ascontiguousarray(row_tag, np.uint32))
            common = dict(buf=d_out, buf_bytes=out_cap, rows=rows, n=n, rec_row=d_row, rec_pos=d_pos, rec_words=words,
                          rec_first=d_first, row_tag=d_tag_in, stride=stride)
            # the size probe (a non-null payload selects the mode; nothing is written through it)
            probe = self.unpack_device(**common, payload=0 if mode == "view" else d_out)
            R, nb = probe["records"], probe["payload_bytes"]
            un = probe
            d_pay = 0
            if R:
                d_off, d_len, d_poff, d_tag = dev(8 * R), dev(4 * R), dev(8 * R), dev(4 * R)
                d_pay = 0 if mode == "view" else dev(nb)
                un = self.unpack_device(**common, offset=d_off, len=d_len, payload_off=d_poff, tag=d_tag, rec_cap=R,
                                        payload=d_pay, payload_cap=0 if mode == "view" else nb)
                if un["status"] != A.RMQ_OK:
                    raise EngineError(un["status"], "rmq_unpack (fetch_columns)")
            cols = {"rec_first": back(d_first, n + 1, np.uint64)}
            for name, p, dt in (("offset", R and d_off, np.uint64), ("len", R and d_len, np.uint32),
                                ("payload_off", R and d_poff, np.uint64), ("tag", R and d_tag, np.uint32)):
                cols[name] = back(p, R, dt)
            cols["unpack"] = un
            if keep_device:
                cols["device"] = dict(buf=d_out, buf_bytes=out_cap, offset=R and d_off, len=R and d_len,
                                      payload_off=R and d_poff, tag=R and d_tag, payload=d_pay, held=list(held))
                held.clear()
            if mode == "view":
                payload = back(d_out, out_cap, np.uint8)
            else:
                payload = back(d_pay, nb if R else 0, np.uint8)
                if stride:
                    payload = payload.reshape(R, stride)
            return res, cols, payload
        finally:
            for p in held:
                self.device_free(p)

    def set_segments(self, pidx, segment_bytes) -> None:
        """Ring sizes of partitions pidx[i] (rmq_set_segments: retention at a smaller size first, the
        retained log keeps its offsets and positions)."""
        p = np.ascontiguousarray(pidx, np.uint32)
        sb = np.ascontiguousarray(segment_bytes, np.uint64)
        _check(self.lib.rmq_set_segments(self.h, len(p), p.ctypes.data_as(C.POINTER(C.c_uint32)),
                                         sb.ctypes.data_as(C.POINTER(C.c_uint64))), "rmq_set_segments")

    # ---- read-back
    def states(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """rmq_get_partition_states: the states of partitions [first, first + n) as a structured
        array of rmq_partition_state (one device copy per field)."""
        n = self.cfg.num_partitions - first if n is None else n
        out = np.zeros(n, STATE_DTYPE)
        _check(self.lib.rmq_get_partition_states(self.h, first, n, _ptr(out)), "rmq_get_partition_states")
        return out

    def state(self, pidx: int) -> dict:
        s = A.RmqPartitionState()
        _check(self.lib.rmq_get_partition_state(self.h, pidx, C.byref(s)), "rmq_get_partition_state")
        return state_to_dict(s, self.cfg.replication_factor)

    def read_segment(self, replica: int, pidx: int, ring_off: int = 0, n: int | None = None) -> np.ndarray:
        n = self.state(pidx)["segment_bytes"] - ring_off if n is None else n
        out = np.empty(n, np.uint8)
        _check(self.lib.rmq_read_segment(self.h, replica, pidx, ring_off, n, _ptr(out)), "rmq_read_segment")
        return out

    def read_index(self, pidx: int, m_first: int, count: int) -> np.ndarray:
        out = np.empty((count, 2), np.uint64)
        _check(self.lib.rmq_read_index(self.h, pidx, m_first, count, _ptr(out)), "rmq_read_index")
        return out

    def consumer_table(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """rmq_read_consumer_table: the consumer-offset rows of partitions [first, first + n)."""
        n = self.cfg.num_partitions - first if n is None else n
        out = np.empty((n, self.cfg.max_consumers), np.uint64)
        _check(self.lib.rmq_read_consumer_table(self.h, first, n, _ptr(out)), "rmq_read_consumer_table")
        return out

    def scrub(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """rmq_scrub: the on-device audit of the retained logs of partitions [first, first + n), every
        local replica slot (FORMAT.md §10): a structured array of rmq_scrub_res, one row per
        partition. Corruption raises nothing (the rows say where it is); self.last_scrub_rc keeps
        the call's return value, RMQ_OK or RMQ_ECORRUPT. Drains first (collective with a transport)."""
        n = self.cfg.num_partitions - first if n is None else n
        out = np.zeros(max(n, 0), SCRUB_RES_DTYPE)
        rc = self.lib.rmq_scrub(self.h, first, n, _ptr(out) if n else None)
        if rc not in (A.RMQ_OK, A.RMQ_ECORRUPT):
            raise EngineError(rc, "rmq_scrub")
        self.last_scrub_rc = rc
        return out

    def repair(self, first: int = 0, n: int | None = None, dry_run: bool = False) -> np.ndarray:
        """rmq_repair: scrub partitions [first, first + n), rewrite every (local slot, segment) pair
        that fails from the lowest local slot on which that segment passes, and scrub again
        (FORMAT.md §10, "Repair"): a structured array of rmq_repair_res, one row per partition.
        dry_run counts what would be rewritten and writes nothing. What remains raises nothing (the
        rows say where it is); self.last_repair_rc keeps the call's return value, RMQ_OK or
        RMQ_ECORRUPT. Drains first (collective with a transport)."""
        n = self.cfg.num_partitions - first if n is None else n
        out = np.zeros(max(n, 0), REPAIR_RES_DTYPE)
        rc = self.lib.rmq_repair(self.h, first, n, A.RMQ_REPAIR_DRY_RUN if dry_run else 0, _ptr(out) if n else None)
        if rc not in (A.RMQ_OK, A.RMQ_ECORRUPT):
            raise EngineError(rc, "rmq_repair")
        self.last_repair_rc = rc
        return out

    def reindex(self, first: int = 0, n: int | None = None, dry_run: bool = False, all: bool = False) -> np.ndarray:
        """rmq_reindex: scrub partitions [first, first + n), rebuild the sparse-index entries of every
        gap (a maximal run of segments that pass on no local slot) by walking the log's records, and
        scrub again (FORMAT.md §10, "Index rebuild"): a structured array of rmq_reindex_res, one row
        per partition. all trusts no stored entry (one walk per partition, from the log start);
        dry_run counts what would be rewritten and writes nothing. What remains raises nothing (the
        rows say where it is); self.last_reindex_rc keeps the call's return value, RMQ_OK or
        RMQ_ECORRUPT. Call it before repair() and repair_remote(). Drains first (collective with a
        transport)."""
        n = self.cfg.num_partitions - first if n is None else n
        flags = (A.RMQ_REINDEX_DRY_RUN if dry_run else 0) | (A.RMQ_REINDEX_ALL if all else 0)
        out = np.zeros(max(n, 0), REINDEX_RES_DTYPE)
        rc = self.lib.rmq_reindex(self.h, first, n, flags, _ptr(out) if n else None)
        if rc not in (A.RMQ_OK, A.RMQ_ECORRUPT):
            raise EngineError(rc, "rmq_reindex")
        self.last_reindex_rc = rc
        return out

    def repair_remote(self, first: int = 0, n: int | None = None, dry_run: bool = False) -> np.ndarray:
        """rmq_repair_remote: repair(), then the pairs it had to leave are fetched from the ranks that
        hold the partition's other replica slots and installed once they verify here (FORMAT.md §10,
        "Remote repair"): a structured array of rmq_repair_remote_res, one row per partition.
        self.last_repair_rc keeps the return value (RMQ_OK or RMQ_ECORRUPT), self.last_repair_served
        the (segments, bytes) this engine sent as a donor. Without a transport it is repair(). With
        one it is collective: every rank calls it, with its own range (n = 0: a donor only)."""
        n = self.cfg.num_partitions - first if n is None else n
        out = np.zeros(max(n, 0), REPAIR_REMOTE_RES_DTYPE)
        served = (C.c_uint64 * 2)()
        rc = self.lib.rmq_repair_remote(self.h, first, n, A.RMQ_REPAIR_DRY_RUN if dry_run else 0,
                                        _ptr(out) if n else None, served)
        if rc not in (A.RMQ_OK, A.RMQ_ECORRUPT):
            raise EngineError(rc, "rmq_repair_remote")
        self.last_repair_rc = rc
        self.last_repair_served = (int(served[0]), int(served[1]))
        return out

    def restore(self, items, buf, rec_pos, dry_run: bool = False, mem: int = A.RMQ_MEM_HOST,
                buf_bytes: int | None = None) -> np.ndarray:
        """rmq_restore: restart pristine partitions from record images (FORMAT.md §11). items: a
        RESTORE_ITEM_DTYPE array; buf: the runs, a uint8 array (mem = RMQ_MEM_HOST) or a device
        address with buf_bytes (RMQ_MEM_DEVICE); rec_pos: the uint64 position table. Returns a
        RESTORE_RES_DTYPE row per item. A refused row raises nothing (its status says why);
        self.last_restore_rc keeps the call's return value. A call-level failure (a transport is
        attached, no memory, a device error) raises. dry_run verifies and writes nothing."""
        items = np.atleast_1d(np.ascontiguousarray(items, RESTORE_ITEM_DTYPE))
        rec_pos = np.ascontiguousarray(rec_pos, np.uint64)
        if mem == A.RMQ_MEM_HOST:
            buf = np.ascontiguousarray(buf, np.uint8)
            bp, nb = (_ptr(buf) if buf.size else None), buf.size
        else:
            bp, nb = buf, int(buf_bytes)
        out = np.zeros(len(items), RESTORE_RES_DTYPE)
        rc = self.lib.rmq_restore(self.h, len(items), _ptr(items) if len(items) else None, mem, bp, nb,
                                  _ptr(rec_pos) if rec_pos.size else None, rec_pos.size,
                                  A.RMQ_RESTORE_DRY_RUN if dry_run else 0, _ptr(out) if len(items) else None)
        if rc and not (len(out) and (out["status"] == rc).any()):
            raise EngineError(rc, "rmq_restore")
        self.last_restore_rc = rc
        return out

    def fault_corrupt_repair(self, dst: int, at: int) -> None:
        """Tests: the next remote-repair response sent to dst has one data byte flipped
        (rmq_fault_corrupt_repair)."""
        _check(self.lib.rmq_fault_corrupt_repair(self.h, dst, at), "rmq_fault_corrupt_repair")

    def fault_flip_ring(self, replica: int, pidx: int, ring_off: int, xor_mask: int = 0x5A) -> None:
        """Tests: XOR one byte of a local replica ring (rmq_fault_flip_ring), addressed as
        read_segment addresses it."""
        _check(self.lib.rmq_fault_flip_ring(self.h, replica, pidx, ring_off, xor_mask), "rmq_fault_flip_ring")

    def fault_flip_index(self, pidx: int, m: int, word: int, xor_mask: int) -> None:
        """Tests: XOR xor_mask into word `word` (0 offset, 1 pos) of index entry m of pidx
        (rmq_fault_flip_index)."""
        _check(self.lib.rmq_fault_flip_index(self.h, pidx, m, word, xor_mask), "rmq_fault_flip_index")

    def consumer_offsets(self, pidx: int) -> np.ndarray:
        out = np.empty(self.cfg.max_consumers, np.uint64)
        _check(self.lib.rmq_read_consumer_offsets(self.h, pidx, _ptr(out)), "rmq_read_consumer_offsets")
        return out

    # ---- device memory / timing
    def device_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(self.lib.rmq_device_alloc(self.h, nbytes, C.byref(p)), "rmq_device_alloc")
        return p.value

    def device_free(self, p: int) -> None:
        _check(self.lib.rmq_device_free(self.h, p), "rmq_device_free")

    def h2d(self, dst: int, src: np.ndarray) -> None:
        src = np.ascontiguousarray(src)
        _check(self.lib.rmq_memcpy(self.h, dst, _ptr(src), src.nbytes, 0), "rmq_memcpy")

    def d2h(self, dst: np.ndarray, src: int) -> None:
        _check(self.lib.rmq_memcpy(self.h, _ptr(dst), src, dst.nbytes, 1), "rmq_memcpy")

    def profile(self, enable: int) -> None:
        """rmq_profile_enable: 0 off, 1 on, k >= 2 on with every fetch's kernels run k times."""
        _check(self.lib.rmq_profile_enable(self.h, int(enable)), "rmq_profile_enable")

    def profile_query(self, kernel: int) -> tuple[int, float]:
        n, ms = C.c_uint64(), C.c_double()
        _check(self.lib.rmq_profile_query(self.h, kernel, C.byref(n), C.byref(ms)), "rmq_profile_query")
        return int(n.value), float(ms.value)

    def device_info(self) -> tuple[str, int]:
        buf = C.create_string_buffer(256)
        cu = C.c_uint32()
        _check(self.lib.rmq_device_info(self.h, buf, 256, C.byref(cu)), "rmq_device_info")
        return buf.value.decode(), int(cu.value)


class LocalHub:
    """rmq_local_hub: in-process transport for `world` engines, each driven by its own thread."""

    def __init__(self, world: int, lib_path: str | None = None):
        self.lib = A.load(lib_path) if lib_path else A.load()
        h = C.c_void_p()
        _check(self.lib.rmq_local_hub_create(world, C.byref(h)), "rmq_local_hub_create")
        self.h = h

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.rmq_local_hub_destroy(self.h)
            self.h = None


def rccl_unique_id() -> bytes:
    buf = (C.c_uint8 * 128)()
    _check(A.load().rmq_rccl_unique_id(buf), "rmq_rccl_unique_id")
    return bytes(buf)


def parse_records(buf: np.ndarray) -> list[tuple[int, int, bytes]]:
    """Split FORMAT.md records: [(offset, crc, payload), ...]."""
    out, pos, b = [], 0, buf.tobytes()
    while pos + 16 <= len(b):
        off = int.from_bytes(b[pos:pos + 8], "little")
        ln = int.from_bytes(b[pos + 8:pos + 12], "little")
        crc = int.from_bytes(b[pos + 12:pos + 16], "little")
        out.append((off, crc, b[pos + 16:pos + 16 + ln]))
        pos += 16 + ((ln + 15) & ~15)
    return out


def table_records(buf: np.ndarray, res: np.ndarray, rec_row: np.ndarray, rec_pos: np.ndarray) -> list:
    """Split a fetch's output with its record table (rmq_fetch_table, FORMAT.md §7 "Record table"):
    one list per request, [(offset, crc, payload), ...] as parse_records gives it for that request's
    run, empty for a request that owns no table words. Every record's position comes from the table
    by array arithmetic: no length word is chained."""
    n = len(res)
    cnt = np.where((res["status"] == A.RMQ_OK) & (res["count"] > 0), res["count"], 0).astype(np.int64)
    total = int(cnt.sum())
    if not total:
        return [[] for _ in range(n)]
    first = np.concatenate(([0], np.cumsum(cnt)))  # records before each request's
    req_of = np.repeat(np.arange(n), cnt)
    k = np.arange(total) - first[req_of]  # ordinal inside the request
    word = np.asarray(rec_row, np.uint64).astype(np.int64)[req_of] + k
    start = res["out_pos"].astype(np.int64)[req_of] + np.asarray(rec_pos, np.uint64).astype(np.int64)[word]
    hdr = np.ascontiguousarray(buf)[start[:, None] + np.arange(16)]  # [total][16] header bytes
    off = hdr[:, :8].copy().view("<u8").ravel()
    ln = hdr[:, 8:12].copy().view("<u4").ravel().astype(np.int64)
    crc = hdr[:, 12:16].copy().view("<u4").ravel()
    lo = start + 16
    b = buf.tobytes()
    recs = [(o, c, b[s:e]) for o, c, s, e in zip(off.tolist(), crc.tolist(), lo.tolist(), (lo + ln).tolist())]
    return [recs[int(first[r]):int(first[r + 1])] for r in range(n)]
