"""Shared by tests/test_fetch_table_model.py and tests/test_gpu_fetch_table.py: the model of
rmq_fetch_table (FORMAT.md §7 "Record table") on the oracle, whose fetch has no table.

The fetch itself is answered by the models there already are (fetch_at_util.model_fetch_at,
fetch_budget_util.model_fetch, fetch_fill_util.model_fill). From the final rows the model derives
w_r (count + 1 for a row served RMQ_OK with records, else 0) and rec_row (its exclusive prefix), and
for every owning row rec_pos from the existing host walk, rmq_scan_records (tier._scan), over that
row's run of the model's output bytes. Every expected value of the GPU tests comes from here.
"""
from __future__ import annotations

import numpy as np

import fetch_at_util as FA
import fetch_budget_util as B
import fetch_fill_util as F
import scrub_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd.tier import _scan

SENT = np.uint64(0xD1D1D1D1D1D1D1D1)  # the fill of table words nothing may write
EDGE_COUNTS = (1, 63, 64, 65, 127, 128, 129, 273)
SWEEP_MAX3 = (1, 63, 64, 65, 127, 128, 129, 1024)


def words_of(res) -> np.ndarray:
    """w_r of the final rows."""
    return np.where((res["status"] == A.RMQ_OK) & (res["count"] > 0), res["count"].astype(np.int64) + 1, 0)


def table_of(res, out):
    """(rec_row [n + 1], rec_pos [rec_row[n]]) of a call answered (res, out)."""
    w = words_of(res)
    rec_row = np.concatenate(([0], np.cumsum(w))).astype(np.uint64)
    rec_pos = np.zeros(int(rec_row[-1]), np.uint64)
    for r in np.flatnonzero(w):
        lo, nb, cnt = int(res["out_pos"][r]), int(res["bytes"][r]), int(res["count"][r])
        k, got, pos = _scan(out[lo:lo + nb], int(res["start_offset"][r]), cnt, False, True)
        assert (k, got) == (cnt, nb), (r, k, got, cnt, nb)
        rec_pos[int(rec_row[r]):int(rec_row[r]) + cnt + 1] = pos.astype(np.uint64)
    return rec_row, rec_pos


def expected(want, rec_cap: int, alloc: int | None = None):
    """(rc, rec_row, rec_pos as the call leaves an array of `alloc` words filled with SENT) for the
    model answer `want` = (rc, rows, output, bytes_used, ...) and a table of rec_cap words."""
    rc, res, out = want[0], want[1], want[2]
    rec_row, rec_pos = table_of(res, out)
    w = words_of(res)
    left = np.full(max(rec_cap, int(rec_row[-1])) if alloc is None else alloc, SENT, np.uint64)
    for r in np.flatnonzero(w):
        a, b = int(rec_row[r]), int(rec_row[r]) + int(w[r])
        if b <= rec_cap:
            left[a:b] = rec_pos[a:b]
    if int(rec_row[-1]) > rec_cap:
        rc = A.RMQ_ENOSPC
    return rc, rec_row, left


def sentinel_arrays(n: int, alloc: int):
    return np.full(n + 1, SENT, np.uint64), np.full(max(alloc, 1), SENT, np.uint64)


def assert_table(got_rc, got_row, got_pos, want, rec_cap: int, what="") -> None:
    """The return code and both table arrays (got_pos: the caller's whole array, SENT-filled before)."""
    rc, rec_row, left = expected(want, rec_cap, alloc=len(got_pos))
    assert got_rc == rc, (what, got_rc, rc)
    assert np.array_equal(got_row, rec_row), (what, np.flatnonzero(got_row != rec_row)[:4])
    bad = np.flatnonzero(got_pos != left)
    assert bad.size == 0, (what, bad[:4], got_pos[bad[:4]], left[bad[:4]])


def kind_of(res, r: int) -> str:
    """The kind of row r: "owning", or which non-owning kind ("empty", "eoffset", "error", "enospc_capacity",
    "enospc_budget", "pending", "corrupt")."""
    s, cnt, rsv = int(res["status"][r]), int(res["count"][r]), int(res["reserved"][r])
    if s == A.RMQ_OK:
        return "owning" if cnt else "empty"
    return {A.RMQ_EOFFSET: "eoffset", A.RMQ_PENDING: "pending", A.RMQ_ECORRUPT: "corrupt"}.get(
        s, ("enospc_budget" if rsv else "enospc_capacity") if s == A.RMQ_ENOSPC else "error")


def reference_walk(run: np.ndarray, count: int) -> np.ndarray:
    """FORMAT.md §7's reference rule over one run: q_0 = 0, q_{k+1} = min(q_k + 16 + align16(len at
    q_k), bytes); words 0 .. count - 1, then the run's bytes."""
    nb, q, w = int(run.size), 0, []
    for _ in range(count):
        w.append(q)
        if q < nb:
            ln = int.from_bytes(run[q + 8:q + 12].tobytes(), "little")
            q = min(q + 16 + ((ln + 15) & ~15), nb)
    return np.array(w + [nb], np.uint64)


# ---- state 1 ----
def plain1(ora, mx):
    """The 32 requests of state 1 without budgets: (rc, rows, output, bytes_used)."""
    pidx, cons = B.all_reqs1()
    return B.model_fetch(ora, pidx, cons, mx, 0)[:4]


def explicit1(ora, mx):
    """fetch_at_util's sweep of explicit offsets on state 1 (88 requests: before the log start, at
    it, inside, at and past the high watermark): ((pidx, consumer, offsets), model answer)."""
    pidx, cons, offs = FA.sweep_reqs1(ora)
    return (pidx, cons, offs), FA.model_fetch_at(ora, pidx, cons, mx, offs)


def fill_caps(full) -> list:
    """Three capacities of fetch_fill_util's sweep for the unbounded answer `full`, around the middle
    row with bytes (r, bytes P_r before it): P_{r+1} - 16 cuts it before its last record, P_r + 1 has
    no room for its first (k* = 0, RMQ_PENDING), P_n - 16 ends inside the call's last row with bytes."""
    P = F.prefix(full[1])
    owners = np.flatnonzero(full[1]["bytes"])
    mid = int(owners[len(owners) // 2])
    caps = [int(P[mid + 1]) - 16, int(P[mid]) + 1, int(P[-1]) - 16]
    assert set(caps) <= set(F.sweep_caps(full[1], full[2]))
    return caps


# ---- state 3: explicit offsets, counts at the lane and window edges ----
def reqs3(ora, cfg, variant: str):
    """(pidx, consumer, max, offsets): every partition at every max of SWEEP_MAX3, from the log start
    ("start"), or shifted so that a record of 1023 B or more is the slice's first ("big_first") or,
    where the log has one far enough in, its last ("big_last")."""
    pidx, mx, offs = [], [], []
    for p in range(U.PARTS3):
        recs = U.host_walk(ora, cfg, 0, p)[2]  # (offset, pos, len) of the retained records
        lo = recs[0][0]
        big = [k for k, x in enumerate(recs) if x[2] >= 1023]
        for m in SWEEP_MAX3:
            k = 0
            if variant == "big_first":
                k = big[(m + p) % len(big)]
            elif variant == "big_last":
                k = next((j - (m - 1) for j in big if j >= m - 1), 0)
            pidx.append(p), mx.append(m), offs.append(lo + k)
    n = len(pidx)
    return np.array(pidx), np.arange(n) % 4, np.array(mx), np.array(offs, np.uint64)


def model3(ora, cfg, variant: str):
    pidx, cons, mx, offs = reqs3(ora, cfg, variant)
    return (pidx, cons, mx, offs), FA.model_fetch_at(ora, pidx, cons, mx, offs)


# ---- state 4: the scan's chunk edges, refused rows between owning ones ----
def reqs4(n: int):
    """fetch_budget_util.reqs4 without budgets, every seventh request naming no partition."""
    pidx, cons, mx, _ = B.reqs4(n)
    pidx = pidx.copy()
    pidx[6::7] += U.P4
    return pidx, cons, mx


def model4(ora, n: int):
    pidx, cons, mx = reqs4(n)
    return (pidx, cons, mx), B.model_fetch(ora, pidx, cons, mx, 0)[:4]
