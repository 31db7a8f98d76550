"""Cost of rmq_lag at BASELINE config B's shape (4,096 partitions, Zipf 1.1, 100 B, RF 3, rings of
1 MiB; 4 consumers per partition lagging the high watermark by U[0, retained records], as bench.py's
fetch leg): one call over the 16,384 (partition, consumer) rows. With rows and result rows in device
memory: the engine's own span of the lag kernel (rmq_profile_query kernel 10: an event before the
kernel to one after it), --reps times; and with ordinary host rows the host's wall time per
synchronous call, profiling off. ONE JSON line reports medians with min-max.

--mode plain uses only calls that exist without rmq_lag, so the same file measures a tree that lacks
it: the yardsticks. The wall time of states() plus consumer_table(), the only lag there is without
the call (records only, two quiescing read-backs, not one snapshot); and the resolve-plus-gather
region (kernel 4) of rmq_fetch over the same rows at max = 1024, device rows and output, replayed
eight times, per run.

    python tools/lag_probe.py [--batches 48] [--reps 20] [--mode both|plain]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripplemq_amd.engine import Engine, EngineConfig  # noqa: E402
from ripplemq_amd.workload import CONFIGS, make_batch  # noqa: E402

REPLAY = 8


def stat(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3), "reps": len(ts)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--mode", default="both", choices=["both", "plain"])
    args = ap.parse_args()
    spec = CONFIGS["B"]
    P, NC = spec.partitions, 4
    cfg = EngineConfig(num_partitions=P, replication_factor=3, segment_bytes=1 << 20, index_interval=1024,
                       max_batch_records=spec.records, max_batch_bytes=16 << 20, pipeline_depth=4, max_consumers=NC)
    n = P * NC
    out = {"tool": "lag_probe", "config": "B", "rows": n, "mode": args.mode}
    with Engine(cfg) as eng:
        pool = [make_batch(spec, q) for q in range(8)]
        for q in range(args.batches):
            b = pool[q % len(pool)]
            eng.append(b.pidx, b.lens, b.payload)
        st = eng.states()
        hw, lo = st["high_watermark"].astype(np.int64), st["log_start_offset"].astype(np.int64)
        g = np.random.default_rng(0x52495050)
        pp, cc = np.repeat(np.arange(P, dtype=np.uint32), NC), np.tile(np.arange(NC, dtype=np.uint32), P)
        behind = (g.random(n) * (np.repeat(hw - lo, NC) + 1)).astype(np.int64)
        eng.commit_consumer_offset(pp, cc, (np.repeat(hw, NC) - behind).astype(np.uint64))
        eng.sync()
        req = np.zeros((n, 4), np.uint32)
        req[:, 0], req[:, 1], req[:, 2] = pp, cc, 1024
        d_req = eng.device_alloc(16 * n)
        eng.h2d(d_req, req.view(np.uint8).reshape(-1))

        # the yardsticks
        walls = []
        for k in range(args.reps + 1):
            t0 = time.perf_counter()
            s2, tab = eng.states(), eng.consumer_table()
            if k:
                walls.append((time.perf_counter() - t0) * 1e6)
        records = np.maximum(np.repeat(s2["high_watermark"].astype(np.int64), NC) - tab.reshape(-1).astype(np.int64), 0)
        out["readback_lag_us"] = stat(walls)
        out["readback_words"] = int(s2.nbytes // 8 + tab.size)
        d_res = eng.device_alloc(32 * n)
        _, _, cap = eng.fetch_device(None, None, None, 0, 0, d_rows=(n, d_req, d_res))  # bytes needed
        d_out = eng.device_alloc(cap)
        regs = []
        for k in range(args.reps + 1):
            eng.profile(REPLAY)
            rc, _, used = eng.fetch_device(None, None, None, d_out, cap, d_rows=(n, d_req, d_res))
            runs, ms = eng.profile_query(4)
            eng.profile(0)
            assert rc == 0 and used == cap and runs == REPLAY
            if k:
                regs.append(ms * 1e3 / runs)
        out["fetch_max1024_region_us"] = stat(regs)
        out["fetch_max1024_bytes"] = int(cap)
        eng.device_free(d_out), eng.device_free(d_res)

        if args.mode == "both":
            from ripplemq_amd.engine import LAG_RES_DTYPE  # (a tree without the call has neither)

            d_lag = eng.device_alloc(64 * n)
            spans = []
            for k in range(args.reps + 1):
                eng.profile(1)
                eng.lag_device(d_req, None, n, d_lag)
                calls, ms = eng.profile_query(10)
                eng.profile(0)
                assert calls == 1
                if k:
                    spans.append(ms * 1e3)
            rows = np.zeros(n, LAG_RES_DTYPE)
            eng.d2h(rows.view(np.uint8), d_lag)
            assert not rows["status"].any() and np.array_equal(rows["records"].astype(np.int64), records)
            walls = []
            for k in range(args.reps + 1):
                t0 = time.perf_counter()
                host = eng.lag(pp, cc)
                if k:
                    walls.append((time.perf_counter() - t0) * 1e6)
            assert host.tobytes() == rows.tobytes()
            out["lag_kernel_us"] = stat(spans)
            out["lag_host_call_us"] = stat(walls)
            out["lag_records"] = int(rows["records"].sum())
            out["lag_bytes"] = int(rows["bytes"].sum())
            out["lag_min_headroom"] = int(rows["headroom"][rows["records"] > 0].min())
            out["readback_over_host_call"] = round(out["readback_lag_us"]["median"] / out["lag_host_call_us"]["median"], 2)
            eng.device_free(d_lag)
        eng.device_free(d_req)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
