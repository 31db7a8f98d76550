"""Shared by tests/test_lag_model.py (CPU) and tests/test_gpu_lag.py: the model of rmq_lag (FORMAT.md §7
"Lag") on the oracle, which has no lag call, and the scenarios and request lists both files use.

model_lag builds every expected row from the oracle's existing read-backs alone: `state` (log start,
log end, high watermark, leadership, ring bytes), `consumer_offsets` (or the replica cursor the
caller set, which the oracle does not read back) and `record_pos` for the two positions. Every
expected value of the GPU tests comes from here; the CPU file shows that the model agrees with the
oracle's own fetch, that the headroom means what FORMAT.md says, and that the request lists hold the
categories they claim.
"""
from __future__ import annotations

import numpy as np

import high_base_util as H
import scrub_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import LAG_RES_DTYPE

NONE = A.RMQ_OFFSET_NONE
TOP = 2 ** 64 - 2  # the largest offset that can be asked for
CATEGORIES = ("below_start", "at_start", "on_boundary", "spanning", "hw-1", "hw", "hw_to_leo", "past_leo", "2^64-2",
              "empty_partition", "never_committed", "enopart", "enotleader", "einval")


def _col(v, n, dtype=np.uint64):
    return np.broadcast_to(np.asarray(v, dtype), (n,)).copy()


def headroom_of(st, start_pos: int, I: int) -> int:
    """FORMAT.md §7 "Lag": max(floor(start_pos / I) I, log_start_pos) + S_p - log_end_pos, 0 for a state
    with more than S_p bytes retained. Python integers."""
    S, lsp, lep = int(st["segment_bytes"]), int(st["log_start_pos"]), int(st["log_end_pos"])
    if lep < lsp or lep - lsp > S:
        return 0
    return max(start_pos // I * I, lsp) + S - lep


def model_lag(ora, pidx, consumer, offsets=None, replica=False, cursor=None) -> np.ndarray:
    """What rmq_lag must answer for these rows, from the oracle. offsets: None, one value or one per
    row (None / RMQ_OFFSET_NONE entries: the table's); replica: one flag or one per row; cursor:
    {partition: replica cursor} as the caller set them (0 where not named, the oracle's start)."""
    n = len(pidx)
    cfg = ora.cfg
    P, C, I = cfg.num_partitions, cfg.max_consumers, cfg.index_interval
    if offsets is None:
        offs = [NONE] * n
    elif np.isscalar(offsets):
        offs = [int(offsets)] * n
    else:
        offs = [NONE if o is None else int(o) for o in offsets]
    rep = _col(replica, n, bool)
    rows = np.zeros(n, LAG_RES_DTYPE)
    rows["headroom"] = NONE
    states = {}
    for r in range(n):
        p, c = int(pidx[r]), int(consumer[r])
        if not 0 <= p < P:
            rows["status"][r] = A.RMQ_ENOPART
            continue
        st = states.get(p) or states.setdefault(p, ora.state(p))
        if not st["is_leader"] and not rep[r]:
            rows["status"][r] = A.RMQ_ENOTLEADER
            continue
        if not 0 <= c < C:
            rows["status"][r] = A.RMQ_EINVAL
            continue
        if offs[r] != NONE:
            off = offs[r]
        elif rep[r]:
            off = int((cursor or {}).get(p, 0))
        else:
            off = int(ora.consumer_offsets(p)[c])
        hw, lso = int(st["high_watermark"]), int(st["log_start_offset"])
        rows["start_offset"][r] = off
        if off >= hw:
            continue
        start = off
        if off < lso:
            rows["status"][r], start = A.RMQ_EOFFSET, lso
            rows["start_offset"][r], rows["evicted"][r] = lso, lso - off
        if hw <= start:
            continue
        sp, ep = ora.record_pos(p, start), ora.record_pos(p, hw)
        rows["records"][r], rows["bytes"][r] = hw - start, ep - sp
        rows["start_pos"][r], rows["end_pos"][r] = sp, ep
        rows["headroom"][r] = headroom_of(st, sp, I)
    return rows


def assert_rows(got, want, what="") -> None:
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (what, diff[:4], got[diff[:4]], want[diff[:4]])


def reqs_array(pidx, consumer, flags=0) -> np.ndarray:
    req = np.zeros((len(pidx), 4), np.uint32)
    req[:, 0], req[:, 1], req[:, 3] = pidx, consumer, flags
    req[:, 2] = 0xDEAD  # max_records is not read
    return req


def snapshot(e):
    """What a lag call must leave as it was: states, the consumer table, the transport's counters."""
    P = e.cfg.num_partitions
    stats = e.replication_stats() if hasattr(e, "replication_stats") else None
    return [e.state(p) for p in range(P)], np.stack([e.consumer_offsets(p) for p in range(P)]), stats


def assert_unchanged(e, snap) -> None:
    now = snapshot(e)
    assert now[0] == snap[0] and np.array_equal(now[1], snap[1]) and now[2] == snap[2]


# ---- categories -------------------------------------------------------------------------------
def _record_size(ora, p, off) -> int:
    return ora.record_pos(p, off + 1) - ora.record_pos(p, off)


def categorize(ora, pidx, consumer, offs, rows, replica=False, committed=()) -> list:
    """The set of CATEGORIES each row falls in (a row may fall in several, or none: an ordinary offset
    inside the log). committed: the (partition, consumer) pairs some commit has named."""
    I, out = ora.cfg.index_interval, []
    for r in range(len(pidx)):
        p, c, s = int(pidx[r]), int(consumer[r]), int(rows["status"][r])
        cats = set()
        if s in (A.RMQ_ENOPART, A.RMQ_ENOTLEADER, A.RMQ_EINVAL):
            cats.add({A.RMQ_ENOPART: "enopart", A.RMQ_ENOTLEADER: "enotleader", A.RMQ_EINVAL: "einval"}[s])
            out.append(cats)
            continue
        st = ora.state(p)
        lso, leo, hw = int(st["log_start_offset"]), int(st["log_end_offset"]), int(st["high_watermark"])
        o = NONE if offs is None or offs[r] is None else int(offs[r])
        if o == NONE:
            if not replica and (p, c) not in committed:
                assert int(rows["start_offset"][r]) in (0, lso)
                cats.add("never_committed")
            o = int(rows["start_offset"][r]) if s == A.RMQ_OK else lso - int(rows["evicted"][r])
        if leo == 0:
            cats.add("empty_partition")
        if s == A.RMQ_EOFFSET:
            assert o < lso and int(rows["evicted"][r]) == lso - o
            cats.add("below_start")
        if o == TOP:
            cats.add("2^64-2")
        if o == hw:
            cats.add("hw")
        if hw < o <= leo and hw < leo:
            cats.add("hw_to_leo")
        if o > leo:
            cats.add("past_leo")
        if int(rows["records"][r]):
            if o == lso:
                cats.add("at_start")
            if o == hw - 1:
                cats.add("hw-1")
            sp = int(rows["start_pos"][r])
            if lso < o and sp % I == 0:
                cats.add("on_boundary")
            rs = _record_size(ora, p, int(rows["start_offset"][r]))
            if (sp + rs) // I - sp // I >= 2:  # the record covers two interval boundaries or more
                cats.add("spanning")
        out.append(cats)
    return out


def count_categories(lists) -> dict:
    c = dict.fromkeys(CATEGORIES, 0)
    for cats in lists:
        for s in cats:
            for x in s:
                c[x] += 1
    return c


# ---- 1: the sweep on state 1 ------------------------------------------------------------------
P1, NC1 = 8, 4


def filled1(make, **kw):
    cfg = U.cfg1(**kw)
    e = make(cfg)
    U.fill1(e)
    return e, cfg


def sweep_reqs1(ora, parts=range(P1)):
    """(pidx, consumer, offsets): every offset in [0, log_end_offset + 2] of every partition, then
    2^64 - 2 and an entry without an offset (consumer 3, which nothing has committed), then the
    error rows state 1 can hold (all its partitions are led): unknown partitions, consumers out of
    range."""
    pidx, cons, offs = [], [], []
    for p in parts:
        leo = int(ora.state(p)["log_end_offset"])
        for o in list(range(leo + 3)) + [TOP, NONE]:
            pidx.append(p), cons.append(3 if o == NONE else len(offs) % NC1), offs.append(o)
    P, C = ora.cfg.num_partitions, ora.cfg.max_consumers
    for p, c in ((P, 0), (P + 1000, 1), (0xFFFFFFFF, C), (0, C), (5, 0xFFFFFFFF)):
        pidx.append(p), cons.append(c), offs.append(len(offs) % 3)
    return np.array(pidx, np.uint32), np.array(cons, np.uint32), np.array(offs, np.uint64)


def commit_rounds1(ora):
    """The sweep's offsets again, but committed: a list of (pidx, consumer, offsets) rounds, each
    committing one offset to every (partition, consumer) pair: round k gives consumer c of
    partition p the offset 4 k + c, until every partition's log_end_offset + 2 is passed."""
    top = max(int(ora.state(p)["log_end_offset"]) for p in range(P1)) + 2
    pp, cc = np.repeat(np.arange(P1, dtype=np.uint32), NC1), np.tile(np.arange(NC1, dtype=np.uint32), P1)
    return [(pp, cc, (NC1 * k + cc).astype(np.uint64)) for k in range(top // NC1 + 1)]


# ---- 2: a high watermark inside the log, and below its start -----------------------------------
LAGGING2 = (4, 5)  # their two other slots on other ranks: only acks commit


def scenario2(e) -> None:
    """State 1 with partitions 4 and 5 replicated to two remote slots: 4's is acked part-way into
    its retained log, 5's never (its high watermark stays 0, below the log start retention set)."""
    for p in LAGGING2:
        e.set_replicas(p, [e.cfg.rank, 1, 2], 0)
    U.fill1(e)
    st = e.state(LAGGING2[0])
    hw = (int(st["log_start_offset"]) + int(st["log_end_offset"])) // 2
    e.ack([LAGGING2[0]], [1], [hw])


def reqs2(ora):
    pidx, cons, offs = sweep_reqs1(ora, LAGGING2)
    return pidx[:-5], cons[:-5], offs[:-5]  # (the error rows are state 1's)


# ---- 3: long records and a wide table ---------------------------------------------------------
def scenario3(e) -> None:
    """State 3; consumer j of every partition committed to log_start + j: 256 consecutive records,
    more than one cycle of LENS3, so a consumer stands at every boundary of a cycle."""
    U.fill3(e)
    C = e.cfg.max_consumers
    assert C > len(U.LENS3)
    for p in range(U.PARTS3):
        lo = int(e.state(p)["log_start_offset"])
        rc, st = e.commit_consumer_offset(np.full(C, p, np.uint32), np.arange(C, dtype=np.uint32),
                                          lo + np.arange(C, dtype=np.uint64))
        assert rc == 0 and not st.any()


def reqs3():
    return np.repeat(np.arange(U.PARTS3, dtype=np.uint32), 256), np.tile(np.arange(256, dtype=np.uint32), U.PARTS3)


# ---- 4: grid edges -----------------------------------------------------------------------------
WG = 16  # rows per workgroup of the lag kernel (kLagRows)
N4 = (1, 2, 3, WG - 1, WG, WG + 1, 255, 256, 257, 2 * U.P4)
FOLLOWED4 = 4  # a partition state 4's engine holds but does not lead


def scenario4(e) -> None:
    U.fill4(e)
    e.set_replicas(FOLLOWED4, [1, e.cfg.rank], 0)


def reqs4():
    """All 5,000 (partition, consumer) pairs; offsets by row index {none, 0, 1, 5, 2^64 - 2}; among
    them every 7th row names an unknown partition and every 11th a consumer out of range (rows 0 to
    2 stay plain: n = 1, 2, 3 are served rows); partition FOLLOWED4's rows are RMQ_ENOTLEADER."""
    r = np.arange(2 * U.P4)
    pidx, cons = (r // 2).astype(np.uint32), (r % 2).astype(np.uint32)
    offs = np.array((NONE, 0, 1, 5, TOP), np.uint64)[r % 5]
    pidx[(r % 7 == 6)] += U.P4
    cons[(r % 11 == 10)] = 2 + r[(r % 11 == 10)] % 3
    return pidx, cons, offs


# ---- 5: past 2^32 ------------------------------------------------------------------------------
HIGH_P = 2


def high_bases(I: int) -> dict:
    return {0: (0, 0), HIGH_P: (2 ** 32 + 5, 2 ** 40 + 4 * I)}


def scenario5(e, bases, ora=None) -> None:
    """Partition HIGH_P restarted at its base (the engine; the oracle stays at 0), then the same
    batches on both: the rings wrap and retention runs."""
    H.rebase(e, bases, ora)
    for b in H.scenario_batches(5, config_index=75):
        for x in (e, ora):
            if x is not None:
                _, st = x.append(b.pidx, b.lens, b.payload)
                assert st["appended"] == len(b.pidx)


def reqs5(ora):
    """Zero-based (pidx, consumer, offsets) over partitions 0 and HIGH_P: every offset from three
    below the log start to two past the log end, and an entry without one."""
    pidx, cons, offs = [], [], []
    for p in (0, HIGH_P):
        st = ora.state(p)
        lo, leo = int(st["log_start_offset"]), int(st["log_end_offset"])
        assert lo > 3, "retention has run"
        for o in list(range(lo - 3, leo + 3)) + [NONE]:
            pidx.append(p), cons.append(len(offs) % 4), offs.append(o)
    return np.array(pidx, np.uint32), np.array(cons, np.uint32), np.array(offs, np.uint64)


def shift_rows(rows, pidx, bases) -> np.ndarray:
    """The zero-based model's rows as the rebased engine answers them: start_offset moved by the
    base offset, both positions by the base position where the row has records; the rest stays."""
    out = rows.copy()
    for r, p in enumerate(pidx):
        dO, dP = bases.get(int(p), (0, 0))
        if int(rows["status"][r]) in (A.RMQ_OK, A.RMQ_EOFFSET):
            out["start_offset"][r] = int(rows["start_offset"][r]) + dO
            if int(rows["records"][r]):
                out["start_pos"][r] = int(rows["start_pos"][r]) + dP
                out["end_pos"][r] = int(rows["end_pos"][r]) + dP
    return out


def shift_offsets(offs, pidx, bases) -> np.ndarray:
    return np.array([o if int(o) == NONE else int(o) + bases.get(int(p), (0, 0))[0] for o, p in zip(offs, pidx)], np.uint64)


# ---- 6: replica rows ---------------------------------------------------------------------------
FOLLOWED1 = 3


def scenario6(e) -> dict:
    """State 1; partition FOLLOWED1 then moves its leadership to rank 1 (this engine keeps slot 1);
    replica cursors at the log start + 2 (the followed one), inside and below the log (led ones).
    Returns the cursors."""
    U.fill1(e)
    e.set_replicas(FOLLOWED1, [1, e.cfg.rank, 2], 0)
    cur = {}
    for p, add in ((FOLLOWED1, 2), (0, 7), (1, -3), (6, 0), (7, 1)):
        cur[p] = max(int(e.state(p)["log_start_offset"]) + add, 0)
    e.set_replica_cursor(np.array(list(cur), np.uint32), np.array(list(cur.values()), np.uint64))
    return cur


# ---- 7: the headroom's edge --------------------------------------------------------------------
def bytes_batch(p: int, sizes, seed: int = 0):
    """One batch for partition p whose records take exactly sizes[k] bytes each (multiples of 16,
    at least 16): payloads of size - 16 bytes."""
    sizes = [int(s) for s in sizes]
    assert all(s >= 16 and s % 16 == 0 for s in sizes), sizes
    lens = np.array([s - 16 for s in sizes], np.uint32)
    payload = np.random.default_rng(7000 + seed).integers(0, 256, int(lens.sum()), dtype=np.uint8)
    return np.full(len(sizes), p, np.uint32), lens, payload


def split_bytes(total: int, batches: int, g) -> list:
    """`total` bytes (a multiple of 16, at least 16 per batch) as `batches` batches of one or two records."""
    assert total % 16 == 0 and total >= 16 * batches
    cuts = sorted(int(x) * 16 for x in g.choice(np.arange(1, total // 16), batches - 1, replace=False)) if batches > 1 else []
    parts = [b - a for a, b in zip([0] + cuts, cuts + [total])]
    out = []
    for s in parts:
        k = int(g.integers(1, s // 16)) * 16 if s >= 32 and g.random() < 0.5 else 0
        out.append([s - k, k] if k else [s])
    return out
