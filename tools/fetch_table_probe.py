"""Cost of the record table (rmq_fetch_table) at BASELINE config B's shape (4,096 partitions, Zipf 1.1,
100 B, RF 3, rings of 1 MiB; 4 consumers per partition lagging the high watermark by
U[0, retained records], as bench.py's fetch leg): one fetch of the 16,384 requests at max = 10 and
at max = 1024, as rmq_fetch ("plain") and as rmq_fetch_table with a device table ("table"); rows,
output and table in device memory, so both serve the same slices and bytes. Timed three ways,
--reps times each, plain and table alternating: the engine's own fetch profile (rmq_profile_query
kernel 4: an event before the ticket's first kernel to one after its last; the plain fetch replayed
eight times back to back, per run; a call with a table runs once), the span of the table kernels
alone (kernel 9: what the table adds on the device), and the host's wall time per synchronous call
with profiling off (what the table adds to the caller). The table is then compared with what it
replaces: rmq_scan_records over every served run of the same output on one host thread (a ctypes
call per run: the same loop with max_records = 0 measures the calls themselves and is subtracted).
ONE JSON line reports medians with min-max.

--long adds one slice of about 10^5 records (one partition, one request) with a table: the serial
walk of one wave.

--mode plain uses only calls that exist without rmq_fetch_table, so the same file measures a tree
that lacks it: the yardstick.

    python tools/fetch_table_probe.py [--batches 48] [--reps 20] [--mode both|plain] [--long]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripplemq_amd import _abi as A  # noqa: E402
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, EngineConfig  # noqa: E402
from ripplemq_amd.workload import CONFIGS, make_batch  # noqa: E402


REPLAY = 8  # runs of a plain fetch's kernels per profiled call (its first run carries dispatch-span events)


def stat(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3), "reps": len(ts)}


def host_scan_us(lib, out: np.ndarray, rows: np.ndarray, reps: int) -> dict:
    """rmq_scan_records over every served run of `out`, one host thread: us per fetch, the loop's
    own call overhead (the same calls with max_records = 0) measured beside it."""
    served = np.flatnonzero((rows["status"] == 0) & (rows["count"] > 0))
    base = out.ctypes.data
    args = [(base + int(rows["out_pos"][r]), int(rows["bytes"][r]), int(rows["start_offset"][r]), int(rows["count"][r]))
            for r in served]
    pos = np.zeros(int(rows["count"].max()) + 1, np.uint64)
    n, nb = C.c_uint64(), C.c_uint64()
    pp, pn, pb = pos.ctypes.data, C.byref(n), C.byref(nb)
    scan, calls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        for a, b, f, c in args:
            lib.rmq_scan_records(a, b, f, c, 0, pp, pn, pb)
        t1 = time.perf_counter()
        for a, b, f, c in args:
            lib.rmq_scan_records(a, b, f, 0, 0, pp, pn, pb)
        t2 = time.perf_counter()
        scan.append((t1 - t0) * 1e6)
        calls.append((t2 - t1) * 1e6)
    return {"runs": len(args), "loop_us": stat(scan), "calls_only_us": stat(calls),
            "walk_us": round(stat(scan)["median"] - stat(calls)["median"], 3)}


def long_slice(reps: int) -> dict:
    """One partition, about 10^5 records of 100 B, one request for all of them."""
    recs, size = 100_000, 100
    cfg = EngineConfig(num_partitions=2, replication_factor=1, segment_bytes=1 << 25, index_interval=1024,
                       max_batch_records=1 << 16, max_batch_bytes=16 << 20, max_consumers=2)
    g = np.random.default_rng(7)
    with Engine(cfg) as eng:
        left = recs
        while left:
            k = min(left, 50_000)
            eng.append(np.zeros(k, np.uint32), np.full(k, size, np.uint32), g.integers(0, 256, k * size, dtype=np.uint8))
            left -= k
        req = np.array([[0, 0, recs, 0]], np.uint32)
        d_req, d_res, d_row, d_pos = (eng.device_alloc(x) for x in (16, 32, 16, 8 * (recs + 1)))
        eng.h2d(d_req, req.view(np.uint8).reshape(-1))
        _, _, cap = eng.fetch_device(None, None, None, 0, 0, d_rows=(1, d_req, d_res))
        d_out = eng.device_alloc(cap)
        tab, reg = [], []
        for k in range(reps + 1):
            eng.profile(1)
            rc, _, used = eng.fetch_device(None, None, None, d_out, cap, d_rows=(1, d_req, d_res), table=(d_row, d_pos, recs + 1))[:3]
            t9, r4 = eng.profile_query(9)[1] * 1e3, eng.profile_query(4)[1] * 1e3
            eng.profile(0)
            assert rc == 0 and used == cap
            if k:
                tab.append(t9), reg.append(r4)
        rows, pos = np.empty(1, FETCH_RES_DTYPE), np.empty(recs + 1, np.uint64)
        eng.d2h(rows.view(np.uint8), d_res), eng.d2h(pos.view(np.uint8), d_pos)
        assert int(rows["count"][0]) == recs and np.array_equal(pos, np.arange(recs + 1, dtype=np.uint64) * 128)
        return {"records": recs, "bytes": int(cap), "table_kernels_us": stat(tab), "fetch_region_us": stat(reg), "split": "none"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mode", default="both", choices=["both", "plain"])
    ap.add_argument("--long", action="store_true")
    args = ap.parse_args()
    spec = CONFIGS["B"]
    P, NC = spec.partitions, 4
    cfg = EngineConfig(num_partitions=P, replication_factor=3, segment_bytes=1 << 20, index_interval=1024,
                       max_batch_records=spec.records, max_batch_bytes=16 << 20, pipeline_depth=4, max_consumers=NC)
    n = P * NC
    out = {"tool": "fetch_table_probe", "config": "B", "requests": n, "mode": args.mode, "replay_plain": REPLAY}
    with Engine(cfg) as eng:
        pool = [make_batch(spec, q) for q in range(8)]
        for q in range(args.batches):
            b = pool[q % len(pool)]
            eng.append(b.pidx, b.lens, b.payload)
        st = eng.states()
        hw, lo = st["high_watermark"].astype(np.int64), st["log_start_offset"].astype(np.int64)
        g = np.random.default_rng(0x52495050)
        pp, cc = np.repeat(np.arange(P, dtype=np.uint32), NC), np.tile(np.arange(NC, dtype=np.uint32), P)
        lag = (g.random(n) * (np.repeat(hw - lo, NC) + 1)).astype(np.int64)
        eng.commit_consumer_offset(pp, cc, (np.repeat(hw, NC) - lag).astype(np.uint64))
        eng.sync()
        d_req, d_res, d_row = (eng.device_alloc(x) for x in (16 * n, 32 * n, 8 * (n + 1)))
        for mx in (10, 1024):
            req = np.zeros((n, 4), np.uint32)
            req[:, 0], req[:, 1], req[:, 2] = pp, cc, mx
            eng.h2d(d_req, req.view(np.uint8).reshape(-1))
            _, _, cap = eng.fetch_device(None, None, None, 0, 0, d_rows=(n, d_req, d_res))  # bytes needed
            rec_cap = cap // 16 + n  # always suffices
            d_out, d_pos = eng.device_alloc(cap), eng.device_alloc(8 * rec_cap)
            res = {}

            def call(table, prof):
                """One call: (fetch region us per run, table kernels' span us, host wall us)."""
                if prof:
                    eng.profile(1 if table else REPLAY)
                kw = {"table": (d_row, d_pos, rec_cap)} if table else {}
                t0 = time.perf_counter()
                rc, _, used = eng.fetch_device(None, None, None, d_out, cap, d_rows=(n, d_req, d_res), **kw)[:3]
                wall = (time.perf_counter() - t0) * 1e6
                reg = t9 = 0.0
                if prof:
                    runs, ms = eng.profile_query(4)
                    reg = ms * 1e3 / runs
                    t9 = eng.profile_query(9)[1] * 1e3 if table else 0.0
                    eng.profile(0)
                    assert runs == (1 if table else REPLAY)
                assert rc == 0 and used == cap, (rc, used, cap)
                rows = np.empty(n, FETCH_RES_DTYPE)
                eng.d2h(rows.view(np.uint8), d_res)
                res[table] = rows
                return reg, t9, wall

            modes = (False, True) if args.mode == "both" else (False,)
            ts = {m: [] for m in modes}
            walls = {m: [] for m in modes}
            for m in modes:  # warm-up: code objects, slots
                call(m, True), call(m, False)
            for _ in range(args.reps):
                for m in modes:
                    ts[m].append(call(m, True))
            for _ in range(args.reps):  # the host's view, profiling off
                for m in modes:
                    walls[m].append(call(m, False)[2])
            rows = res[False]
            leg = {"bytes": int(cap), "records": int(rows["count"].sum()),
                   "plain_us": stat([t[0] for t in ts[False]]), "plain_call_us": stat(walls[False])}
            if args.mode == "both":
                assert np.array_equal(res[False], res[True])  # the same slices and bytes
                leg["table_us"] = stat([t[0] for t in ts[True]])
                leg["table_call_us"] = stat(walls[True])
                leg["table_kernels_us"] = stat([t[1] for t in ts[True]])
                leg["table_minus_plain_us"] = round(leg["table_us"]["median"] - leg["plain_us"]["median"], 3)
                leg["table_minus_plain_call_us"] = round(leg["table_call_us"]["median"] - leg["plain_call_us"]["median"], 3)
                # the table against the host walk it replaces, over the same output
                host_out, row, pos = np.empty(cap, np.uint8), np.empty(n + 1, np.uint64), np.empty(rec_cap, np.uint64)
                eng.d2h(host_out, d_out), eng.d2h(row.view(np.uint8), d_row), eng.d2h(pos.view(np.uint8), d_pos)
                served = np.flatnonzero((rows["status"] == 0) & (rows["count"] > 0))
                r = int(served[len(served) // 2])  # one run checked here; the tests check them all
                want = np.zeros(int(rows["count"][r]) + 1, np.uint64)
                k, nb = C.c_uint64(), C.c_uint64()
                A.load().rmq_scan_records(host_out.ctypes.data + int(rows["out_pos"][r]), int(rows["bytes"][r]),
                                          int(rows["start_offset"][r]), int(rows["count"][r]), 0, want.ctypes.data,
                                          C.byref(k), C.byref(nb))
                assert np.array_equal(pos[int(row[r]):int(row[r + 1])], want), r
                assert int(row[n]) == int(rows["count"].sum()) + len(served)
                leg["table_words"] = int(row[n])
                leg["host_scan"] = host_scan_us(A.load(), host_out, rows, max(3, args.reps // 4))
                leg["host_walk_over_table_kernels"] = round(leg["host_scan"]["walk_us"] / leg["table_kernels_us"]["median"], 2)
                leg["host_walk_over_call_difference"] = round(
                    leg["host_scan"]["walk_us"] / max(leg["table_minus_plain_call_us"], 1e-3), 2)
            out[f"max{mx}"] = leg
            eng.device_free(d_out), eng.device_free(d_pos)
    if args.long and args.mode == "both":
        out["long_slice"] = long_slice(args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
