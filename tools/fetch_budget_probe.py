"""Cost of the fetch trim kernel (rmq_fetch_bytes) at BASELINE config B's shape (4,096 partitions,
Zipf 1.1, 100 B, RF 3, rings of 1 MiB; 4 consumers per partition lagging the high watermark by
U[0, retained records], as bench.py's fetch leg): one fetch of the 16,384 requests at max = 1024
with a budget of --budget bytes each (rows, budgets and output in device memory), beside an
unbudgeted fetch of the same state whose max_records are the counts the budgeted one returned, so
both return the same bytes. Each is timed by the engine's own fetch profile (rmq_profile_query
kernel 4: an event before the ticket's first kernel to one after its last), --reps times, and ONE
JSON line reports the medians (with min-max) and their difference, the trim kernel's cost. The
unbudgeted fetch is timed twice: as one run, which carries the profile's dispatch-span events
between its two kernels, and replayed eight times back to back (per run), which does not.

    python tools/fetch_budget_probe.py [--batches 48] [--reps 20] [--budget 4096]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, EngineConfig  # noqa: E402
from ripplemq_amd.workload import CONFIGS, make_batch  # noqa: E402


def stat(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "reps": len(ts)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--budget", type=int, default=4096)
    args = ap.parse_args()
    spec = CONFIGS["B"]
    P, NC = spec.partitions, 4
    cfg = EngineConfig(num_partitions=P, replication_factor=3, segment_bytes=1 << 20, index_interval=1024,
                       max_batch_records=spec.records, max_batch_bytes=16 << 20, pipeline_depth=4, max_consumers=NC)
    n = P * NC
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
        cap = n * args.budget
        d_out, d_req, d_res, d_bud = (eng.device_alloc(x) for x in (cap, 16 * n, 32 * n, 4 * n))
        req = np.zeros((n, 4), np.uint32)
        req[:, 0], req[:, 1], req[:, 2] = pp, cc, 1024
        eng.h2d(d_req, req.view(np.uint8).reshape(-1))
        eng.h2d(d_bud, np.full(n, args.budget, np.uint32).view(np.uint8))
        res = np.empty(n, FETCH_RES_DTYPE)

        def timed(rows, replay=1):
            # (an unbudgeted ticket's single run carries the dispatch-span events of profile kernel
            # 3 between its two kernels; replayed k times only the first run does. A budgeted
            # ticket runs once, without them.)
            eng.profile(replay)
            rc, _, used = eng.fetch_device(None, None, None, d_out, cap, d_rows=rows)
            runs, ms = eng.profile_query(4)
            eng.profile(0)
            assert rc == 0 and runs == replay, (rc, runs)
            return ms * 1e3 / runs, used

        _, used_b = timed((n, d_req, d_res, d_bud))
        eng.d2h(res.view(np.uint8), d_res)
        trimmed = int(((res["status"] == 0) & (res["count"] < 1024) & (res["bytes"] > args.budget - 144)).sum())
        nospc = int((res["status"] != 0).sum())
        req2 = req.copy()
        req2[:, 2] = res["count"]  # the same bytes, unbudgeted
        d_req2 = eng.device_alloc(16 * n)
        eng.h2d(d_req2, req2.view(np.uint8).reshape(-1))
        _, used_u = timed((n, d_req2, d_res))
        tb, tu, tr = [], [], []
        for _ in range(args.reps):  # alternating, after the warm-up pair above
            tb.append(timed((n, d_req, d_res, d_bud))[0])
            tu.append(timed((n, d_req2, d_res))[0])
            tr.append(timed((n, d_req2, d_res), 8)[0])
        sb, su = stat(tb), stat(tu)
        print(json.dumps({"tool": "fetch_budget_probe", "config": "B", "requests": n, "max_records": 1024,
                          "budget": args.budget, "bytes_budgeted": used_b, "bytes_unbudgeted_same_counts": used_u,
                          "rows_near_budget": trimmed, "rows_budget_enospc": nospc,
                          "records": int(res["count"].sum()),
                          "budgeted_us": sb, "unbudgeted_us": su, "unbudgeted_replay8_us_per_run": stat(tr),
                          "trim_cost_us": sb["median"] - su["median"],
                          "trim_cost_vs_replay_us": sb["median"] - stat(tr)["median"]}))


if __name__ == "__main__":
    main()
