"""Shared by tests/test_fetch_fill_model.py and tests/test_gpu_fetch_fill.py: the model of
RMQ_FETCH_FILL (FORMAT.md §7 "Filling a bounded output") on the oracle, whose fetch has no fill.

The model answers the call with an unlimited output first (fetch_budget_util.model_fetch, or
fetch_at_util.model_fetch_at with explicit offsets: budgets and offsets applied, nothing committed),
reads every row's bytes B_r, finds the crossing request r* (the first with P_r + B_r > out_cap) and
its cut k* from the record sizes of its slice, runs the same model again on the rows that are not
pending only (zero-byte rows move no out_pos, so the subset's out_pos are the whole call's), with
k* as r*'s max_records and `commit` as asked, and writes the pending rows and a k* = 0 row in by
hand. Every expected value of the GPU tests comes from here.
"""
from __future__ import annotations

import numpy as np

import fetch_at_util as FA
import fetch_budget_util as B
import scrub_util as U
from ripplemq_amd import _abi as A

CATEGORIES = ("whole", "cut_mid", "cut_boundary", "cut_zero_pending", "cut_zero_enospc", "pending", "passthrough",
              "fits")
SWEEP_MAX = B.SWEEP_MAX
P1, NC1 = B.P1, B.NC1


def _model(ora, pidx, cons, mx, bud, offs, out_cap=None, commit=False, replica=False):
    """(rc, rows, output, bytes_used) of the call without the flag."""
    if offs is None:
        return B.model_fetch(ora, pidx, cons, mx, bud, out_cap=out_cap, commit=commit, replica=replica)[:4]
    return FA.model_fetch_at(ora, pidx, cons, mx, offs, max_bytes=bud, out_cap=out_cap, commit=commit, replica=replica)


def unbounded(ora, pidx, consumer, max_records, max_bytes=None, replica=False, offsets=None):
    """The call answered with an unlimited out_cap, nothing committed (model_fill's first step; a
    sweep of capacities over one call computes it once and passes it on)."""
    n = len(pidx)
    bud = B.broadcast(0 if max_bytes is None else max_bytes, n)
    offs = None if offsets is None else B.broadcast(offsets, n)
    return _model(ora, np.asarray(pidx), np.asarray(consumer), B.broadcast(max_records, n), bud, offs, replica=replica)


def prefix(res) -> np.ndarray:
    """P_0 .. P_n of an unbounded answer."""
    return np.concatenate(([0], np.cumsum(res["bytes"].astype(np.uint64)))).astype(np.int64)


def model_fill(ora, pidx, consumer, max_records, max_bytes, out_cap, commit=False, replica=False, offsets=None,
               full=None):
    """What a fetch with RMQ_FETCH_FILL must answer: (rc, rows, output bytes, bytes_used, category of
    every request). full: unbounded(...) of the same call, if the caller has it."""
    n = len(pidx)
    pidx, cons = np.asarray(pidx), np.asarray(consumer)
    mx = B.broadcast(max_records, n)
    bud = B.broadcast(0 if max_bytes is None else max_bytes, n)
    offs = None if offsets is None else B.broadcast(offsets, n)
    if full is None:
        full = _model(ora, pidx, cons, mx, bud, offs, replica=replica)
    _, res0, out0, used0 = full
    nb = res0["bytes"].astype(np.int64)
    assert not nb[(res0["status"] != A.RMQ_OK) | (res0["count"] == 0)].any()
    P = prefix(res0)
    assert int(P[n]) == used0
    cap = int(out_cap)
    if used0 <= cap:  # everything fits: exactly the call without the flag
        rc, res, out, used = _model(ora, pidx, cons, mx, bud, offs, out_cap=cap, commit=commit, replica=replica)
        assert rc == A.RMQ_OK and used == used0
        return rc, res, out, used, ["fits"] * n
    rs = int(np.flatnonzero(P[1:] > cap)[0])  # r*: the first request that crosses the end (it has bytes)
    assert nb[rs] > 0 and P[rs] <= cap < P[rs] + nb[rs]
    room = cap - int(P[rs])
    lo = int(res0["out_pos"][rs])
    cum = np.cumsum(B.record_sizes(out0[lo:lo + int(nb[rs])]))
    assert cum.size == int(res0["count"][rs])
    k = int(np.searchsorted(cum, room, side="right"))
    assert k < cum.size
    pending = (np.arange(n) > rs) & (nb > 0)
    keep = ~pending
    if k == 0:
        keep[rs] = False
    cats = ["whole"] * rs + ["?"] + ["pending" if pending[r] else "passthrough" for r in range(rs + 1, n)]
    cats[rs] = ("cut_zero_enospc" if P[rs] == 0 else "cut_zero_pending") if k == 0 else \
        "cut_boundary" if int(cum[k - 1]) == room else "cut_mid"
    sel = np.flatnonzero(keep)
    res = np.zeros(n, res0.dtype)
    out, used = np.zeros(1, np.uint8), 0
    if sel.size:
        mxs = mx.copy()
        mxs[rs] = k  # (r* with k = 0 is not among the rows kept)
        rc, res_s, out, used = _model(ora, pidx[sel], cons[sel], mxs[sel], bud[sel], None if offs is None else offs[sel],
                                      commit=commit, replica=replica)
        assert rc == A.RMQ_OK
        res[sel] = res_s
    assert used == int(P[rs]) + (int(cum[k - 1]) if k else 0) <= cap
    for r in np.flatnonzero(~keep):
        res["start_offset"][r] = res0["start_offset"][r]
        res["status"][r] = A.RMQ_PENDING
        res["out_pos"][r] = used
    if k == 0:  # not even its first record fits
        res["out_pos"][rs], res["reserved"][rs] = P[rs], cum[0]
        if P[rs] == 0:
            res["status"][rs] = A.RMQ_ENOSPC  # the output itself is too small: the capacity that would do
    return A.RMQ_OK, res, out, used, cats


def sweep_caps(res0, out0) -> list:
    """The capacities of the state 1 sweep for one unbounded answer: 0, 15, 16, every P_r, P_r -+ 16,
    P_r + 1, P_r + the first record's size of request r and that minus 16, P_n - 16, P_n, P_n + 16."""
    P = prefix(res0)
    n = len(res0)
    caps = {0, 15, 16, int(P[n]) - 16, int(P[n]), int(P[n]) + 16}
    for r in range(n):
        p, nb = int(P[r]), int(res0["bytes"][r])
        caps |= {p, p - 16, p + 16, p + 1}
        if nb:
            first = int(B.record_sizes(out0[p:p + nb])[0])
            caps |= {p + first, p + first - 16}
    return sorted(c for c in caps if c >= 0)


def sweep1(ora) -> dict:
    """The sweep on state 1 (all 32 requests): {max: (unbounded answer, {cap: model_fill})}."""
    pidx, cons = B.all_reqs1()
    out = {}
    for mx in SWEEP_MAX:
        full = unbounded(ora, pidx, cons, mx)
        out[mx] = (full, {cap: model_fill(ora, pidx, cons, mx, None, cap, full=full)
                          for cap in sweep_caps(full[1], full[2])})
    return out


def count_categories(models) -> dict:
    c = dict.fromkeys(CATEGORIES, 0)
    for m in models:
        for x in m[4]:
            c[x] += 1
    return c


def check_properties(want, full, out_cap) -> None:
    """What holds of every model answer by construction (confirmed by the CPU tests)."""
    rc, res, out, used, cats = want
    _, res0, out0, used0 = full
    assert rc == A.RMQ_OK and used <= max(int(out_cap), 0) and used == int(res["bytes"].sum())
    served = np.flatnonzero((res["status"] == A.RMQ_OK) & (res["bytes"] > 0))
    pos = 0
    for r in served:  # the served bytes are contiguous from 0
        assert int(res["out_pos"][r]) == pos
        pos += int(res["bytes"][r])
    assert pos == used
    assert not ((res["status"] == A.RMQ_ENOSPC) & (res["reserved"] == 0)).any()  # never a capacity RMQ_ENOSPC
    if cats[0] == "fits":
        assert np.array_equal(res, res0) and used == used0
        return
    rs = next(r for r, c in enumerate(cats) if c.startswith("cut"))
    assert np.array_equal(res[:rs], res0[:rs])  # every row before r* equals the unbounded answer
    assert np.array_equal(out[:int(res["out_pos"][rs])], out0[:int(res0["out_pos"][rs])])
    for r in range(rs + 1, len(res)):
        if cats[r] == "pending":
            assert res[r] == np.array([(res0["start_offset"][r], used, 0, 0, A.RMQ_PENDING, 0)], res.dtype)[0]
        else:
            assert cats[r] == "passthrough" and int(res["bytes"][r]) == 0 and int(res["out_pos"][r]) == used
            assert all(res[f][r] == res0[f][r] for f in ("start_offset", "count", "status", "reserved"))


# ---- state 4: the gather workgroup and chunk edges ----
RSTAR4 = (0, 15, 16, 17, 255, 256, 257, 511, 512)


def targets4(n: int) -> list:
    """The requests r* falls on in a call of n requests: the edges of RSTAR4 and n - 1."""
    return sorted({r for r in RSTAR4 + (n - 1,) if r < n})


def reqs4(n: int, shift: int, budgets: bool):
    """fetch_budget_util.reqs4 with the partitions rotated by `shift` (state 4's partitions hold
    records or none by p mod 3: some rotation of 0, 1, 2 puts records under any request index)."""
    pidx, cons, mx, bud = B.reqs4(n)
    return (pidx + shift) % U.P4, cons, mx, (bud if budgets else None)


def calls4(ora, n: int, budgets: bool):
    """[(r*, shift, out_cap, unbounded answer)] of state 4's calls of n requests: for every target a
    rotation under which it has bytes and a capacity that ends inside them; then (None, 0, P_n, .)."""
    fulls, out = {}, []

    def full(s):
        if s not in fulls:
            pidx, cons, mx, bud = reqs4(n, s, budgets)
            fulls[s] = unbounded(ora, pidx, cons, mx, bud)
        return fulls[s]

    for r in targets4(n):
        s = next(s for s in range(3) if int(full(s)[1]["bytes"][r]) > 0)
        res0 = full(s)[1]
        out.append((r, s, int(prefix(res0)[r]) + (int(res0["bytes"][r]) // 2 & ~15), full(s)))
    out.append((None, 0, full(0)[3], full(0)))
    return out


# ---- state 3: the cut walks index entries and a large record ----
def edge_calls3(ora, cfg):
    """(pidx, consumer, max, unbounded answer, j, capacities): 256 requests of one record each but
    request j > 0, which asks for two, the second a record of 4,096 B or more; the capacities put
    fetch_budget_util.edge_calls3's six edges (s_j - 16, s_j - 1, s_j, s_j + 1, s_j + s_{j+1} - 16,
    s_j + s_{j+1}) on the crossing request, as its budget out_cap - P_j."""
    calls, big, s = B.edge_calls3(ora, cfg)
    j = int(np.flatnonzero(big & (np.arange(B.NC3) > 0))[0])
    assert int(s[j + 1]) >= 4096
    pidx, cons = np.full(B.NC3, B.P3), np.arange(B.NC3)
    mx = np.where(np.arange(B.NC3) == j, 2, 1)
    full = unbounded(ora, pidx, cons, mx)
    assert int(full[1]["bytes"][j]) == int(s[j] + s[j + 1])
    return pidx, cons, mx, full, j, [int(prefix(full[1])[j]) + int(calls[k][j]) for k in range(6)]


assert_equals_model = B.assert_equals_model
