"""Shared by tests/test_fetch_at_model.py and tests/test_gpu_fetch_at.py: the model of rmq_fetch_at
(FORMAT.md §7 "Explicit offsets") on the oracle, whose fetch reads from committed offsets only.

A fetch at offset o must answer as the oracle's fetch does after the oracle's
commit_consumer_offset(p, c, o). The model therefore maps every explicit request to a scratch
consumer id of its own (the same partition; SCRATCH0 + k for the k-th explicit request of that
partition in the call, so no other request of the call reads or writes that (partition, id) row,
and the table needs as many scratch columns as one partition has explicit requests, not as the
call has: state 4's 2,500 partitions would otherwise carry 2,500 columns each), commits the
request's offset there, runs ONE batched oracle fetch of all the requests (through
fetch_budget_util.model_fetch when budgets are given), and puts the table rows back. Requests with
RMQ_OFFSET_NONE keep their consumer id. RMQ_FETCH_REPLICA requests move the oracle's replica
cursor the same way (one request per partition). With commit=True the model then writes the
committing requests' next offsets where the engine must have written them, so the oracle stays in
step with the engine. Every expected value of the GPU tests comes from here.

The oracle and the engine are made with the same config, whose max_consumers leaves room for the
scratch ids above the consumers the tests use (SCRATCH0 and up).
"""
from __future__ import annotations

import dataclasses

import numpy as np

import fetch_budget_util as B
import scrub_util as U
from ripplemq_amd import _abi as A

NONE = A.RMQ_OFFSET_NONE
P1, NC1 = B.P1, B.NC1
SCRATCH0 = 8  # the first scratch consumer id: the tests' own consumers are below it

SWEEP_MAX = (1, 10, 0xFFFFFFFF)
KINDS = ("0", "start-1", "start", "start+1", "middle", "hw-1", "hw", "hw+1", "2^32+5", "2^64-2", "none")
CATEGORIES = ("eoffset", "served_from_start", "served_inside", "served_last", "empty_at_hw", "empty_past_hw",
              "empty_far", "saturating", "none")
N_SWEEP = P1 * len(KINDS)


def cfg1(n_scratch: int = len(KINDS)):
    return U.cfg1(max_consumers=SCRATCH0 + n_scratch)


def filled1(make, n_scratch: int = len(KINDS)):
    """State 1 with fetch_budget_util's four consumer offsets per partition, and room for scratch ids."""
    cfg = cfg1(n_scratch)
    e = make(cfg)
    U.fill1(e)
    B.commit_offsets(e, cfg)
    return e, cfg


def offsets_of(st) -> list:
    """The sweep's offsets of a partition in state st, in the order of KINDS."""
    lo, hw = int(st["log_start_offset"]), int(st["high_watermark"])
    return [0, (lo - 1) % 2 ** 64, lo, lo + 1, lo + (hw - lo) // 2, (hw - 1) % 2 ** 64, hw, hw + 1, 2 ** 32 + 5,
            2 ** 64 - 2, NONE]


def sweep_reqs1(ora):
    """(pidx, consumer, offsets) of the sweep: every partition at every kind of offset, 88 requests
    in one call (several non-committing explicit requests per (partition, consumer))."""
    pidx = np.repeat(np.arange(P1), len(KINDS))
    cons = np.tile(np.arange(len(KINDS)) % NC1, P1)
    offs = np.array([o for p in range(P1) for o in offsets_of(ora.state(p))], np.uint64)
    return pidx, cons, offs


def _replica_cursor(ora, p: int) -> int:
    _, res, _, _ = ora.fetch([p], [0], [0], replica=True)  # an empty slice starts at the cursor
    assert int(res["status"][0]) == A.RMQ_OK, res
    return int(res["start_offset"][0])


def model_fetch_at(ora, pidx, consumer, max_records, offsets, max_bytes=None, out_cap=None, commit=False,
                   replica=False):
    """What rmq_fetch_at must answer, from the oracle: (rc, rows, output bytes, bytes_used)."""
    n = len(pidx)
    pidx, consumer = np.asarray(pidx, np.int64), np.asarray(consumer, np.int64)
    offs = B.broadcast(NONE if offsets is None else offsets, n)
    P, C = ora.cfg.num_partitions, ora.cfg.max_consumers
    explicit = [r for r in range(n) if int(offs[r]) != NONE and 0 <= pidx[r] < P]
    cons = consumer.copy()
    saved_rows, saved_cur = {}, {}
    if replica:
        parts = [int(pidx[r]) for r in explicit]
        assert len(set(parts)) == len(parts), "one explicit replica request per partition"
        for r in explicit:
            p = int(pidx[r])
            saved_cur[p] = _replica_cursor(ora, p)
            ora.set_replica_cursor([p], [int(offs[r])])
    else:
        assert (consumer[consumer < C] < SCRATCH0).all()
        for r in explicit:
            p = int(pidx[r])
            if not 0 <= consumer[r] < C:
                continue  # refused whatever the offset: keeps its id
            row = saved_rows.setdefault(p, {})
            cons[r] = SCRATCH0 + len(row)
            assert cons[r] < C, (p, len(row), C)
            row[int(cons[r])] = int(ora.consumer_offsets(p)[cons[r]])
            ora.commit_consumer_offset([p], [int(cons[r])], [int(offs[r])])  # (refused where the fetch is)
    try:
        if max_bytes is None:
            rc, res, out, used = ora.fetch(pidx, cons, max_records, out_cap=out_cap, commit=commit, replica=replica)
        else:
            rc, res, out, used = B.model_fetch(ora, pidx, cons, max_records, max_bytes, out_cap=out_cap, commit=commit,
                                               replica=replica)[:4]
    finally:
        for p, row in saved_rows.items():
            ora.commit_consumer_offset(np.full(len(row), p, np.uint32), np.array(list(row), np.uint32),
                                       np.array(list(row.values()), np.uint64))
        for p, cur in saved_cur.items():
            ora.set_replica_cursor([p], [cur])
    if commit:  # the explicit requests' commits, where the engine makes them
        for r in explicit:
            s = int(res["status"][r])
            if s not in (A.RMQ_OK, A.RMQ_EOFFSET):
                continue
            nx = int(res["start_offset"][r]) + (int(res["count"][r]) if s == A.RMQ_OK else 0)
            if replica:
                ora.set_replica_cursor([int(pidx[r])], [nx])
            else:
                ora.commit_consumer_offset([int(pidx[r])], [int(consumer[r])], [nx])
    return rc, res, out, used


def categorize(ora, pidx, max_records, offs, res) -> list:
    """The category of every request of a sweep call (exactly one each; anything else raises)."""
    mx = B.broadcast(max_records, len(pidx))
    cats = []
    for r, p in enumerate(pidx):
        st = ora.state(int(p))
        lo, hw = int(st["log_start_offset"]), int(st["high_watermark"])
        o, m = int(offs[r]), int(mx[r])
        s, start, cnt = int(res["status"][r]), int(res["start_offset"][r]), int(res["count"][r])
        if o == NONE:
            cats.append("none")
        elif s == A.RMQ_EOFFSET:
            assert o < lo and start == lo and cnt == 0
            cats.append("eoffset")
        elif s == A.RMQ_OK and cnt > 0:
            assert lo <= o < hw and start == o and cnt == min(m, hw - o)
            cats.append("served_from_start" if o == lo else "served_last" if o + cnt == hw else "served_inside")
        elif s == A.RMQ_OK:
            assert o >= hw and start == o and int(res["bytes"][r]) == 0
            cats.append("saturating" if o + m >= 2 ** 64 else "empty_at_hw" if o == hw else
                        "empty_past_hw" if o <= hw + 1 else "empty_far")
        else:
            raise AssertionError(("unexpected row", r, res[r]))
    return cats


def sweep1(ora) -> dict:
    """The sweep on state 1: {max: (model_fetch_at of the 88 requests, their categories)}."""
    pidx, cons, offs = sweep_reqs1(ora)
    out = {}
    for mx in SWEEP_MAX:
        want = model_fetch_at(ora, pidx, cons, mx, offs)
        out[mx] = (want, categorize(ora, pidx, mx, offs, want[1]))
    return out


def count_categories(sweep) -> dict:
    c = dict.fromkeys(CATEGORIES, 0)
    for _, cats in sweep.values():
        for x in cats:
            c[x] += 1
    return c


# ---- state 4: the edges of the LDS-staged load (16 rows per resolve workgroup, 256 per chunk) ----
def reqs4(n: int):
    """(pidx, consumer, max, offsets) of the first n partitions, consumer 0; the explicit offsets
    alternate {0, 1, RMQ_OFFSET_NONE} by request index."""
    r = np.arange(n)
    return r, np.zeros(n, np.uint32), np.full(n, 1024), np.array((0, 1, NONE), np.uint64)[r % 3]


def cfg4():
    return dataclasses.replace(U.cfg4(), max_consumers=SCRATCH0 + 1)  # one explicit request per partition


def tables(e) -> np.ndarray:
    return np.stack([e.consumer_offsets(p) for p in range(e.cfg.num_partitions)])


assert_equals_model = B.assert_equals_model
