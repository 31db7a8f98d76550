"""Shared by tests/test_fetch_budget_model.py and tests/test_gpu_fetch_budget.py: the model of
rmq_fetch_bytes (FORMAT.md §7 "Byte budgets") on the oracle, whose fetch has no budgets.

The model runs the oracle's unbudgeted fetch, reads the record sizes of every served slice from its
bytes, computes k* (the largest number of the slice's records whose bytes are at most the budget),
runs the oracle's fetch again with max_records = k* for the requests that are cut, and substitutes
the RMQ_ENOSPC row for k* = 0. Every expected value of the GPU tests comes from here.
"""
from __future__ import annotations

import numpy as np

import scrub_util as U
from ripplemq_amd import _abi as A
from test_gpu_fetch_verify import _commit_offsets as commit_offsets  # (importing it needs no GPU)

# the sweep of the issue: state 1 (scrub_util), the four consumer offsets per partition of
# test_gpu_fetch_verify._commit_offsets, these max_records and these budgets
SWEEP_MAX = (1, 10, 1024)
SWEEP_BUDGETS = (1, 15, 16, 17, 31, 32, 255, 256, 257, 272, 512, 1520, 4096, 0xFFFFFFFF)
CATEGORIES = ("zero", "one", "mid", "boundary", "untrimmed", "untrimmed_equal", "empty")
P1, NC1 = 8, 4


def filled1(make):
    """State 1 with the four consumer offsets per partition (log start, inside, near the end, the
    end); make(cfg) creates the engine (GPU or oracle)."""
    cfg = U.cfg1()
    e = make(cfg)
    U.fill1(e)
    commit_offsets(e, cfg)
    return e, cfg


def all_reqs1():
    return np.repeat(np.arange(P1), NC1), np.tile(np.arange(NC1), P1)


def record_sizes(buf: np.ndarray) -> np.ndarray:
    """Sizes (16 + align16(len)) of the FORMAT.md §1 records that fill buf."""
    out, pos, n = [], 0, buf.size
    while pos < n:
        ln = int.from_bytes(buf[pos + 8:pos + 12].tobytes(), "little")
        out.append(16 + ((ln + 15) & ~15))
        pos += out[-1]
    assert pos == n
    return np.array(out, np.uint64)


def broadcast(v, n) -> np.ndarray:
    return np.broadcast_to(np.asarray(v, np.uint64), (n,)).copy()


def model_fetch(ora, pidx, consumer, max_records, max_bytes, out_cap=None, commit=False, replica=False):
    """What rmq_fetch_bytes must answer, from the oracle: (rc, rows, output bytes, bytes_used,
    category of every request, k* of every request). out_cap None: sized to fit."""
    n = len(pidx)
    mx, bud = broadcast(max_records, n), broadcast(max_bytes, n)
    _, res0, b0, _ = ora.fetch(pidx, consumer, mx, replica=replica)  # unbudgeted, sized to fit, no commit
    kstar, first, cats = mx.copy(), np.zeros(n, np.uint64), []
    for r in range(n):
        cnt, nb, b = int(res0["count"][r]), int(res0["bytes"][r]), int(bud[r])
        if int(res0["status"][r]) != A.RMQ_OK or cnt == 0:
            cats.append("empty")
        elif b == 0 or nb <= b:
            cats.append("untrimmed_equal" if nb == b else "untrimmed")
        else:
            lo = int(res0["out_pos"][r])
            cum = np.cumsum(record_sizes(b0[lo:lo + nb]))
            assert cum.size == cnt
            k = int(np.searchsorted(cum, b, side="right"))
            assert k < cnt
            kstar[r], first[r] = k, min(int(cum[0]), nb)
            cats.append("zero" if k == 0 else "one" if k == 1 else "boundary" if int(cum[k - 1]) == b else "mid")
    rc, res, out, used = ora.fetch(pidx, consumer, kstar, out_cap=out_cap, commit=commit, replica=replica)
    res = res.copy()
    for r in range(n):
        if cats[r] == "zero":  # the oracle answered max_records = 0: an empty slice at the same place
            assert (int(res["status"][r]), int(res["count"][r]), int(res["bytes"][r])) == (A.RMQ_OK, 0, 0)
            res["status"][r], res["reserved"][r] = A.RMQ_ENOSPC, first[r]
    return rc, res, out, used, cats, kstar


def sweep1(ora):
    """The sweep on state 1: {(max, budget): model_fetch of all 32 requests with that budget}."""
    pidx, cons = all_reqs1()
    return {(mx, b): model_fetch(ora, pidx, cons, mx, b) for mx in SWEEP_MAX for b in SWEEP_BUDGETS}


def count_categories(results) -> dict:
    c = dict.fromkeys(CATEGORIES, 0)
    for r in results:
        for x in r[4]:
            c[x] += 1
    return c


# ---- state 4: grid and chunk edges (2,500 partitions, consumer 0 at offset 0) ----
N4 = (1, 15, 16, 17, 255, 256, 257, 2500)
BUDGETS4 = (0, 144, 1000)


def reqs4(n: int):
    """(pidx, consumer, max, budgets) of the first n partitions; the budgets alternate so that
    every class of partition (by p mod 3: empty, one to three records, 10 to 25) meets each."""
    r = np.arange(n)
    return r, np.zeros(n, np.uint32), np.full(n, 1024), np.array(BUDGETS4, np.uint64)[(r + r // 3) % 3]


# ---- state 3: cut-point edges (I = 1024, one partition, consumer j at log_start + j) ----
P3 = 1          # the partition the 256 consumers read
NC3 = 256


def commit_offsets3(e, cfg) -> None:
    lo = e.state(P3)["log_start_offset"]
    rc, st = e.commit_consumer_offset(np.full(NC3, P3, np.uint32), np.arange(NC3, dtype=np.uint32),
                                      lo + np.arange(NC3, dtype=np.uint64))
    assert rc == 0 and not st.any()


def filled3(make):
    cfg = U.cfg3()
    e = make(cfg)
    U.fill3(e)
    commit_offsets3(e, cfg)
    return e, cfg


def sizes3(ora, cfg) -> np.ndarray:
    """Record sizes of partition P3's retained log, from the log start."""
    recs = U.host_walk(ora, cfg, 0, P3)[2]
    return np.array([16 + ((ln + 15) & ~15) for _, _, ln in recs], np.uint64)


def edge_calls3(ora, cfg):
    """The budget arrays of state 3's calls (256 requests each, consumer j, max = 0xFFFFFFFF):
    the six edges around s_j and s_j + s_{j+1}, then s_j + 1024 i (i = 0..17) for the consumers one
    record before a record of 4,096 B or more (every other request s_j: one record, so that no
    call copies 256 whole logs)."""
    s = sizes3(ora, cfg)
    assert s.size > NC3 + 1
    sj, sn = s[:NC3], s[1:NC3 + 1]
    calls = [sj - 16, sj - 1, sj, sj + 1, sj + sn - 16, sj + sn]
    big = sn >= 4096
    for i in range(18):
        calls.append(np.where(big, sj + 1024 * i, sj))
    return calls, big, s


def assert_equals_model(got, want, what="") -> None:
    """got = (rc, rows, output, bytes_used) of the engine; want = model_fetch(...)."""
    rc, res, out, used = got
    assert (rc, used) == (want[0], want[3]), (what, rc, used, want[0], want[3])
    diff = np.flatnonzero(res != want[1])
    assert diff.size == 0, (what, diff[:4], res[diff[:4]], want[1][diff[:4]])
    for r in np.flatnonzero((res["status"] == A.RMQ_OK) & (res["bytes"] > 0)):
        lo, hi = int(res["out_pos"][r]), int(res["out_pos"][r]) + int(res["bytes"][r])
        assert np.array_equal(out[lo:hi], want[2][lo:hi]), (what, r)
