"""The argument contract of the append path (rmq_append, rmq_ticket_stats, rmq_poll_commit), of
rmq_commit_consumer_offset and rmq_ack, and the roles of the launches a fixed script of appends makes,
called through the C library with raw pointers so that nulls and bad counts reach it.

What is pinned: which error a refused call answers when several apply, that a refused append takes no
ticket and leaves every partition's state as it was (the bytes of rmq_get_partition_states), the
tickets whose stats stay readable, what a consumer-offset call answers per item and as a whole, and the
`rmq launch` lines of RMQ_TRACE=1 (batches and workgroups per role of every launch) for the default
knobs, five knob settings and rank 0 of a two-rank LocalHub. The lines were recorded on an MI355X
(256 CUs) from the library before the append host path moved out of engine.cpp.

With 4 partitions and at most 3 tasks per group, RMQ_WG3_ALL=0 and RMQ_S3_LEAD=5 leave the lines as
the default's (stage 3 has one workgroup either way, and the lead count is not printed): those two
cases pin that the knob changes nothing it must not, not that it arrives; what each knob does to a
grid is tools/launch_plan_main.cpp's part.

Rules other tests pin already (not repeated here):
  device payload addresses, lengths and ranges at their edges            test_gpu_append_device
  page-locked batches                                                      test_gpu_pinned
  configurations rmq_create refuses                                        test_abi
  what the knobs' launches compute, against the oracle                     test_gpu_parity, test_gpu_stage*
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import sys
import tempfile
import threading

import numpy as np
import pytest

from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine, EngineConfig, LocalHub

pytestmark = pytest.mark.gpu

P, RF, NC, SEG, IVL, NMAX, BMAX = 4, 1, 2, 1 << 14, 64, 64, 4096
STATS_RING = 64  # kStatsRing: tickets whose stats stay readable
OK, PENDING, EINVAL, ENOPART, ENOSPC, ENOTLEADER = (A.RMQ_OK, A.RMQ_PENDING, A.RMQ_EINVAL, A.RMQ_ENOPART,
                                                    A.RMQ_ENOSPC, A.RMQ_ENOTLEADER)
HOST, DEVICE, PINNED = A.RMQ_MEM_HOST, A.RMQ_MEM_DEVICE, A.RMQ_MEM_PINNED
UNSET = 0xABCD0000ABCD  # a ticket word no call wrote
CUS = 256  # the CU count the launch lines were recorded at


def _cfg(rank=0, rf=RF):
    return EngineConfig(num_partitions=P, replication_factor=rf, segment_bytes=SEG, index_interval=IVL,
                        max_consumers=NC, max_batch_records=NMAX, max_batch_bytes=BMAX, pipeline_depth=2, rank=rank)


def _a(x):  # an array's address, or null
    return None if x is None else x.ctypes.data


def u32(*v):
    return np.array(v, np.uint32)


def u64(*v):
    return np.array(v, np.uint64)


def host_batch(n, rec=8):
    """n records of `rec` bytes over the partitions in turn: (pidx, lens, payload, out)."""
    return ((np.arange(n) % P).astype(np.uint32), np.full(n, rec, np.uint32),
            (np.arange(n * rec) % 251).astype(np.uint8), np.zeros(max(n, 1), np.uint64))


def raw_append(e, n, mem, pidx, lens, poff, payload, nbytes, out, h="engine", b="batch", t="ticket"):
    """rmq_append with exactly these pointers; h / b / t = None pass a null engine / batch / ticket."""
    bat = A.RmqBatch(n, mem, _a(pidx), _a(lens), _a(poff), payload if isinstance(payload, (int, type(None))) else
                     _a(payload), nbytes)
    tk = C.c_uint64(UNSET)
    rc = e.lib.rmq_append(e.h if h else None, C.byref(bat) if b else None, _a(out), C.byref(tk) if t else None)
    return rc, tk.value


def accepted(e, n=0):
    """An accepted host batch of n records, applied: its ticket."""
    pidx, lens, pay, out = host_batch(n)
    rc, t = raw_append(e, n, HOST, pidx, lens, None, pay if n else None, pay.size, out)
    assert rc == OK and t != UNSET, (rc, t)
    e.sync()
    return t


def snap(e):
    return e.states(0, P).tobytes()


def stats_of(e, ticket):
    st = A.RmqAppendStats()
    rc = e.lib.rmq_ticket_stats(e.h, ticket, C.byref(st))
    return rc, {f: int(getattr(st, f)) for f, _ in A.RmqAppendStats._fields_}


@pytest.fixture(scope="module")
def eng():
    with Engine(_cfg()) as e:
        assert accepted(e, 12) == 1  # three records in every partition
        yield e


def test_fixture_shape(eng):
    s = eng.states()
    assert list(s["is_leader"]) == [1] * P and list(s["log_end_offset"]) == [3] * P == list(s["commit"])
    rc, st = stats_of(eng, 1)
    assert rc == OK and st["records"] == 12 == st["appended"]


def test_append_error_precedence(eng):
    e = eng
    pidx, lens, pay, out = host_batch(4)
    big = host_batch(NMAX + 1)
    t0 = accepted(e)
    before = snap(e)
    cases = [
        # nulls first
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=32, out=out, h=None)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=32, out=out, b=None)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=32, out=out, t=None)),
        # the batch's size before its memory kind and before its pointers
        (ENOSPC, dict(n=NMAX + 1, mem=99, pidx=big[0], lens=big[1], poff=None, payload=pay, nbytes=32, out=big[3])),
        (ENOSPC, dict(n=4, mem=99, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=BMAX + 1, out=out)),
        (ENOSPC, dict(n=NMAX + 1, mem=HOST, pidx=None, lens=None, poff=None, payload=None, nbytes=32, out=None)),
        (ENOSPC, dict(n=0, mem=HOST, pidx=None, lens=None, poff=None, payload=None, nbytes=BMAX + 1, out=None)),
        (EINVAL, dict(n=4, mem=99, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=32, out=out)),
        (EINVAL, dict(n=4, mem=3, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=32, out=out)),
        # then the pointers
        (EINVAL, dict(n=4, mem=HOST, pidx=None, lens=lens, poff=None, payload=pay, nbytes=32, out=out)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=None, poff=None, payload=pay, nbytes=32, out=out)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=32, out=None)),
        (EINVAL, dict(n=4, mem=PINNED, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=32, out=None)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=None, payload=None, nbytes=32, out=out)),
        (EINVAL, dict(n=0, mem=HOST, pidx=None, lens=None, poff=None, payload=None, nbytes=1, out=None)),
        # host ranges: a record past the payload's end, by its running offset or by an explicit one
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=None, payload=pay, nbytes=31, out=out)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=u64(0, 8, 16, 25), payload=pay, nbytes=32, out=out)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=u64(0, 8, 16, 33), payload=pay, nbytes=32, out=out)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=lens, poff=u64(0, 8, 1 << 63, 24), payload=pay, nbytes=32,
                      out=out)),
        (EINVAL, dict(n=4, mem=HOST, pidx=pidx, lens=u32(8, 8, 0xFFFFFFFF, 8), poff=None, payload=pay, nbytes=32,
                      out=out)),
    ]
    for want, kw in cases:
        rc, t = raw_append(e, **kw)
        assert rc == want and t == UNSET, (rc, want, t, kw)
    assert snap(e) == before
    assert accepted(e) == t0 + 1  # no refused call took a ticket


def test_append_misaligned_device_payload(eng):
    e = eng
    d = e.device_alloc(256)
    try:
        t0 = accepted(e)
        before = snap(e)
        for off in (1, 2, 3):
            bat = A.RmqBatch(1, DEVICE, d, d + 16, None, d + 64 + off, 8)
            tk = C.c_uint64(UNSET)
            assert e.lib.rmq_append(e.h, C.byref(bat), d + 32, C.byref(tk)) == EINVAL and tk.value == UNSET, off
        # the size and the null pointers are looked at before the alignment
        bat = A.RmqBatch(NMAX + 1, DEVICE, d, d + 16, None, d + 65, 8)
        assert e.lib.rmq_append(e.h, C.byref(bat), d + 32, C.byref(tk)) == ENOSPC
        assert snap(e) == before and accepted(e) == t0 + 1
    finally:
        e.device_free(d)


def test_append_zero_length_record_at_the_end(eng):
    """A record of length 0 may sit at off == payload_bytes (and its offset is not looked at at all)."""
    e = eng
    pidx, lens, pay, out = host_batch(4)
    lens = u32(8, 8, 8, 0)
    for poff in (None, u64(0, 8, 16, 24), u64(0, 8, 16, 99)):  # (None: running offsets, the last one is 24)
        rc, t = raw_append(e, 4, HOST, pidx, lens, poff, pay, 24, out)
        assert rc == OK, poff
        e.sync()
        rc, st = stats_of(e, t)
        assert rc == OK and st["records"] == 4 == st["appended"] and st["rejected_invalid"] == 0, st


def test_ticket_stats(eng):
    e = eng
    st = A.RmqAppendStats()
    assert e.lib.rmq_ticket_stats(None, 1, C.byref(st)) == EINVAL
    assert e.lib.rmq_ticket_stats(e.h, 1, None) == EINVAL
    first = accepted(e, 5)
    for _ in range(STATS_RING - 2):
        accepted(e)
    last = accepted(e)
    assert last == first + STATS_RING - 1
    assert stats_of(e, 0)[0] == EINVAL
    assert stats_of(e, last + 1)[0] == EINVAL      # never issued
    assert stats_of(e, A.RMQ_TICKET_OFFSETS | 1)[0] == EINVAL
    rc, s = stats_of(e, first)                     # exactly kStatsRing - 1 behind: still answers
    assert rc == OK and s["records"] == 5 == s["appended"], s
    rc, s = stats_of(e, last)                      # an empty batch
    assert rc == OK and all(v == 0 for v in s.values()), s
    assert accepted(e) == last + 1
    assert stats_of(e, first)[0] == EINVAL         # kStatsRing behind
    assert stats_of(e, first + 1)[0] == OK


def test_poll_commit(eng):
    e, poll = eng, eng.lib.rmq_poll_commit
    last = accepted(e)
    assert poll(None, 0, None, None) == EINVAL
    assert poll(e.h, last + 1, None, None) == EINVAL   # never issued
    assert poll(e.h, 0, None, None) == OK
    assert poll(e.h, last, None, None) == OK
    commit, hw = np.zeros(P, np.uint64), np.zeros(P, np.uint64)
    assert poll(e.h, 0, _a(commit), None) == OK and poll(e.h, last, None, _a(hw)) == OK
    assert np.array_equal(commit, e.states()["commit"]) and np.array_equal(hw, e.states()["high_watermark"])
    # consumer-offset tickets: unknown ones, and one polled twice
    assert poll(e.h, A.RMQ_TICKET_OFFSETS | 0x123456, None, None) == EINVAL
    assert poll(e.h, A.RMQ_TICKET_OFFSETS, None, None) == EINVAL
    rc, st = e.commit_consumer_offset([0], [0], [1])
    tk = e.last_offset_ticket
    assert rc == OK and tk & A.RMQ_TICKET_OFFSETS and tk != A.RMQ_TICKET_OFFSETS
    assert poll(e.h, tk, None, None) == OK             # one replica: on its quorum as soon as it ran
    assert poll(e.h, tk, None, None) == EINVAL         # resolved already


def raw_commit(e, pidx, cons, off, n, status=True, ticket=True):
    st = np.full(max(n, 1), 77, np.int32)
    tk = C.c_uint64(UNSET)
    rc = e.lib.rmq_commit_consumer_offset(e.h, _a(pidx), _a(cons), _a(off), n, _a(st) if status else None,
                                          C.byref(tk) if ticket else None)
    return rc, list(st[:n]), tk.value


def test_commit_consumer_offset(eng):
    e = eng
    assert e.lib.rmq_commit_consumer_offset(None, None, None, None, 0, None, None) == EINVAL
    assert raw_commit(e, None, None, None, 0) == (OK, [], 0)          # n = 0: the ticket comes back 0
    assert raw_commit(e, u32(0), u32(0), u64(1), 0) == (OK, [], 0)
    for nul in range(3):                                                # a null array with n > 0
        arrs = [u32(0), u32(0), u64(1)]
        arrs[nul] = None
        assert raw_commit(e, *arrs, 1) == (EINVAL, [77], 0)
    # partition 3 placed on another rank: not led here
    assert e.lib.rmq_set_placement(e.h, 1, _a(u32(3)), None, _a(u32(1)), _a(u32(0))) == OK
    try:
        assert e.state(3)["is_leader"] == 0
        # per item: the partition, then its leadership, then the consumer; the call answers its first
        # failing item in call order
        rc, st, tk = raw_commit(e, u32(3, P, 1, 0, 3), u32(0, 0, NC, 1, NC), u64(1, 1, 1, 2, 1), 5)
        assert (rc, st) == (ENOTLEADER, [ENOTLEADER, ENOPART, EINVAL, OK, ENOTLEADER]) and tk & A.RMQ_TICKET_OFFSETS
        rc, st, tk = raw_commit(e, u32(0, 0xFFFFFFFF, 3), u32(NC, 0, 0), u64(1, 1, 1), 3)
        assert (rc, st, tk) == (EINVAL, [EINVAL, ENOPART, ENOTLEADER], 0)   # nothing accepted: no ticket
        rc, st, tk = raw_commit(e, u32(P, 0), u32(0, 0), u64(1, 3), 2, status=False, ticket=False)
        assert rc == ENOPART
        assert list(e.consumer_offsets(0)) == [3, 2]
        # the same (partition, consumer) several times: the last offset stays
        rc, st, tk = raw_commit(e, u32(1, 1, 2, 1, 1), u32(1, 1, 0, 0, 1), u64(1, 3, 1, 3, 2), 5)
        assert (rc, st) == (OK, [OK] * 5)
        assert list(e.consumer_offsets(1)) == [3, 2] and list(e.consumer_offsets(2)) == [1, 0]
    finally:
        assert e.lib.rmq_set_placement(e.h, 1, _a(u32(3)), None, _a(u32(0)), _a(u32(0))) == OK
        assert e.lib.rmq_become_leader(e.h, 3, e.state(3)["term"] + 1) == OK


def test_ack(eng):
    e, ack = eng, eng.lib.rmq_ack
    assert ack(None, None, None, None, 0) == EINVAL
    assert ack(e.h, None, None, None, 0) == OK
    before = snap(e)
    one = (u32(0), u32(0), u64(1))
    for nul in range(3):
        arrs = [_a(x) for x in one]
        arrs[nul] = None
        assert ack(e.h, *arrs, 1) == EINVAL
    # per item the partition before the slot; the first bad item in call order answers
    assert ack(e.h, _a(u32(P)), _a(u32(RF)), _a(u64(1)), 1) == ENOPART
    assert ack(e.h, _a(u32(0, P)), _a(u32(RF, 0)), _a(u64(1, 1)), 2) == EINVAL
    assert ack(e.h, _a(u32(P, 0)), _a(u32(0, RF)), _a(u64(1, 1)), 2) == ENOPART
    assert ack(e.h, _a(u32(0, 1, P)), _a(u32(0, 0, 0)), _a(u64(3, 3, 3)), 3) == ENOPART  # nothing applied
    assert snap(e) == before


# ---- the roles of every launch (RMQ_TRACE)

SCRIPT = (3, 64, 0, 33, 64, 1)  # records of the six batches: groups of 2 + 1, 0 + 1 and 1 + 1 tiles


@contextlib.contextmanager
def stderr_lines(out):
    """The process's stderr (file descriptor 2: the library writes there) into `out`, line by line."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            yield
        finally:
            sys.stderr.flush()
            os.dup2(saved, 2)
            os.close(saved)
            f.seek(0)
            out.extend(f.read().decode(errors="replace").splitlines())


def run_script(e):
    keep = []
    for n in SCRIPT:
        pidx, lens, pay, out = host_batch(n)
        keep.append((pidx, lens, pay, out))
        rc, _ = raw_append(e, n, HOST, pidx if n else None, lens if n else None, None, pay if n else None, pay.size,
                           out if n else None)
        assert rc == OK, (rc, n)
    e.sync()
    return keep


def traced(knob=None, hub=False):
    """The `rmq launch` lines of the script: on a single engine, or on rank 0 of a two-rank LocalHub
    with two replicas of every partition, so that rank 0 leads partitions with a remote replica and runs
    the 512-thread kernel (rank 1, created without RMQ_TRACE, makes the same calls)."""
    env = {"RMQ_TRACE": "1", **({knob[0]: knob[1]} if knob else {})}
    old = {k: os.environ.get(k) for k in env}
    lines, engs, h = [], [], None
    with stderr_lines(lines):
        try:
            os.environ.update(env)
            engs.append(Engine(_cfg(0, 2 if hub else RF)))
            cus = engs[0].device_info()[1]
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        try:
            if hub:
                h = LocalHub(2)
                engs.append(Engine(_cfg(1, 2)))
                errs = []

                def body(r):
                    try:
                        engs[r].attach_local(h)
                        engs[r].set_placement(np.arange(P), 10 + np.arange(P, dtype=np.uint64),
                                              np.array([[0, 1], [0, 1], [1, 0], [1, 0]], np.uint32), np.zeros(P, np.uint32))
                        run_script(engs[r])
                    except BaseException as ex:  # noqa: BLE001 - reported below
                        errs.append((r, ex))

                ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(2)]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join(120)
                    assert not t.is_alive(), "a rank hung"
                assert not errs, errs
            else:
                run_script(engs[0])
        finally:
            for e in engs:
                e.close()
            if h:
                h.close()
    return cus, [ln for ln in lines if ln.startswith("rmq launch")]


# (long lines: each is one line of the library's output, kept whole)
TRACE = {
    "default": [
        "rmq launch 1: s1 2 batches 2 wgs | s2 0 batches 0 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 2: s1 2 batches 1 wgs | s2 2 batches 1 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 3: s1 2 batches 2 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 0 batches",
        "rmq launch 4: s1 0 batches 0 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 2 batches",
        "rmq launch 5: s1 0 batches 0 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 2 batches",
    ],
    "RMQ_WG3_ALL=0": [
        "rmq launch 1: s1 2 batches 2 wgs | s2 0 batches 0 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 2: s1 2 batches 1 wgs | s2 2 batches 1 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 3: s1 2 batches 2 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 0 batches",
        "rmq launch 4: s1 0 batches 0 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 2 batches",
        "rmq launch 5: s1 0 batches 0 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 2 batches",
    ],
    "RMQ_S3_LEAD=5": [
        "rmq launch 1: s1 2 batches 2 wgs | s2 0 batches 0 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 2: s1 2 batches 1 wgs | s2 2 batches 1 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 3: s1 2 batches 2 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 0 batches",
        "rmq launch 4: s1 0 batches 0 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 2 batches",
        "rmq launch 5: s1 0 batches 0 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 2 batches",
    ],
    "RMQ_S3_ROLES=1": [
        "rmq launch 1: s1 2 batches 2 wgs | s2 0 batches 0 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 2: s1 2 batches 1 wgs | s2 2 batches 1 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 3: s1 2 batches 2 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 3 wgs + 2048 big | s4 0 batches",
        "rmq launch 4: s1 0 batches 0 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 2 wgs + 2048 big | s4 2 batches",
        "rmq launch 5: s1 0 batches 0 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 2 batches 3 wgs + 2048 big | s4 2 batches",
    ],
    "RMQ_S1_WGS=1": [
        "rmq launch 1: s1 2 batches 1 wgs | s2 0 batches 0 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 2: s1 2 batches 1 wgs | s2 2 batches 1 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 3: s1 2 batches 1 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 0 batches",
        "rmq launch 4: s1 0 batches 0 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 2 batches",
        "rmq launch 5: s1 0 batches 0 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 2 batches 1 wgs + 2048 big | s4 2 batches",
    ],
    "RMQ_BIG_WGS=3": [
        "rmq launch 1: s1 2 batches 2 wgs | s2 0 batches 0 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 2: s1 2 batches 1 wgs | s2 2 batches 1 wgs | parts 0 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 3: s1 2 batches 2 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 3 big | s4 0 batches",
        "rmq launch 4: s1 0 batches 0 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 3 big | s4 2 batches",
        "rmq launch 5: s1 0 batches 0 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 2 batches 1 wgs + 3 big | s4 2 batches",
    ],
    "hub": [
        "rmq launch 1: s1 2 batches 2 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 2: s1 2 batches 1 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 0 batches 0 wgs + 0 big | s4 0 batches",
        "rmq launch 3: s1 2 batches 2 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 1024 big | s4 0 batches",
        "rmq launch 4: s1 0 batches 0 wgs | s2 2 batches 1 wgs | parts 1 wgs | s3 2 batches 1 wgs + 1024 big | s4 2 batches",
        "rmq launch 5: s1 0 batches 0 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 2 batches 1 wgs + 1024 big | s4 2 batches",
        "rmq launch 6: s1 0 batches 0 wgs | s2 0 batches 0 wgs | parts 1 wgs | s3 0 batches 0 wgs + 0 big | s4 2 batches",
    ],
}


@pytest.mark.parametrize("case", ["default", "RMQ_WG3_ALL=0", "RMQ_S3_LEAD=5", "RMQ_S3_ROLES=1", "RMQ_S1_WGS=1",
                                  "RMQ_BIG_WGS=3", "hub"])
def test_launch_roles(case):
    knob = tuple(case.split("=")) if "=" in case else None
    cus, lines = traced(knob, hub=case == "hub")
    assert cus == CUS, f"the launch lines were recorded at {CUS} CUs, this device has {cus}"
    assert lines == TRACE[case], "\n".join(lines)
