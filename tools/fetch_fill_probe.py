"""Cost of filling a bounded output (RMQ_FETCH_FILL) at BASELINE config B's shape (4,096 partitions,
Zipf 1.1, 100 B, RF 3, rings of 1 MiB; 4 consumers per partition lagging the high watermark by
U[0, retained records], as bench.py's fetch leg): one fetch of the 16,384 requests at max = 10 and
at max = 1024 (rows, budgets and output in device memory), four ways:

  plain       rmq_fetch, out_cap = the bytes needed (P_n)
  fill_fits   RMQ_FETCH_FILL, out_cap = P_n: the fill kernel finds every chunk inside
  fill_half   RMQ_FETCH_FILL, out_cap = P_n / 2: half the chunks served, one cut, half put off
  share_half  rmq_fetch_bytes, out_cap = P_n / 2, every request's budget an equal share of it

A filling call is never replayed, so every variant is timed as ONE call by the engine's own fetch
profile (rmq_profile_query kernel 4: an event before the ticket's first kernel to one after its
last, rmq_profile_enable(1)); `plain` also replayed eight times back to back, per run, as
tools/fetch_at_probe.py times it (a single plain run records dispatch spans, which hold its second
kernel back: the replayed figure is the one to compare kernels with). --reps repetitions,
alternating; ONE JSON line reports the medians with min-max.

--spill: passes and seconds of DurableLog(spill_bytes=N) with and without fill=True on the same
Zipf state after --spill-batches batches, N an eighth of the backlog, against the unbounded spill.

    python tools/fetch_fill_probe.py [--batches 48] [--reps 20] [--spill] [--spill-batches 4]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripplemq_amd import tier as T  # noqa: E402
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, EngineConfig  # noqa: E402
from ripplemq_amd.workload import CONFIGS, make_batch  # noqa: E402

REPLAY = 8
VARIANTS = ("plain", "plain_replayed", "fill_fits", "fill_half", "share_half")


def stat(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3), "reps": len(ts)}


def config(spec, NC):
    return EngineConfig(num_partitions=spec.partitions, replication_factor=3, segment_bytes=1 << 20, index_interval=1024,
                        max_batch_records=spec.records, max_batch_bytes=16 << 20, pipeline_depth=4, max_consumers=NC)


def fetch_cost(args, spec, NC) -> dict:
    P = spec.partitions
    n = P * NC
    out = {}
    with Engine(config(spec, NC)) as eng:
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
        d_req, d_res, d_bud = (eng.device_alloc(x) for x in (16 * n, 32 * n, 4 * n))
        for mx in (10, 1024):
            req = np.zeros((n, 4), np.uint32)
            req[:, 0], req[:, 1], req[:, 2] = pp, cc, mx
            eng.h2d(d_req, req.view(np.uint8).reshape(-1))
            _, _, need = eng.fetch_device(None, None, None, 0, 0, d_rows=(n, d_req, d_res))  # bytes needed (P_n)
            half = need // 2 & ~15
            eng.h2d(d_bud, np.full(n, half // n & ~15, np.uint32).view(np.uint8))
            d_out = eng.device_alloc(need)
            seen = {}

            def timed(v):
                replay = REPLAY if v == "plain_replayed" else 1
                eng.profile(replay)
                if v in ("plain", "plain_replayed"):
                    rc, _, used = eng.fetch_device(None, None, None, d_out, need, d_rows=(n, d_req, d_res))
                elif v == "share_half":
                    rc, _, used = eng.fetch_device(None, None, None, d_out, half, d_rows=(n, d_req, d_res, d_bud))
                else:
                    rc, _, used = eng.fetch_device(None, None, None, d_out, need if v == "fill_fits" else half,
                                                   d_rows=(n, d_req, d_res), fill=True)
                runs, ms = eng.profile_query(4)
                eng.profile(0)
                assert rc == 0 and runs == replay, (v, rc, runs)
                rows = np.empty(n, FETCH_RES_DTYPE)
                eng.d2h(rows.view(np.uint8), d_res)
                seen[v] = (rows, int(used))
                return ms * 1e3 / runs

            ts = {v: [] for v in VARIANTS}
            for v in VARIANTS:  # warm-up: code objects, slots
                timed(v)
            for _ in range(args.reps):
                for v in VARIANTS:
                    ts[v].append(timed(v))
            assert np.array_equal(seen["plain"][0], seen["fill_fits"][0]) and seen["fill_fits"][1] == need
            rows, used = seen["fill_half"]
            assert half - 16 * 1024 < used <= half and (rows["status"] == 1).any()
            leg = {"bytes_needed": int(need), "out_cap_half": int(half),
                   "fill_half": {"bytes_used": used, "served": int(((rows["status"] == 0) & (rows["bytes"] > 0)).sum()),
                                 "pending": int((rows["status"] == 1).sum())},
                   "share_half": {"bytes_used": seen["share_half"][1]}}
            for v in VARIANTS:
                leg[v + "_us"] = stat(ts[v])
            out[f"max{mx}"] = leg
            eng.device_free(d_out)
    return out


def spill_cost(args, spec) -> dict:
    P = spec.partitions
    parts = range(P)
    out = {}
    with Engine(config(spec, 4)) as eng:
        for q in range(args.spill_batches):
            b = make_batch(spec, q)
            eng.append(b.pidx, b.lens, b.payload)
        eng.sync()
        st = eng.states()
        starts = st["log_start_offset"].astype(np.int64)
        root = tempfile.mkdtemp(prefix="rmq_fill_probe_", dir=os.environ.get("RMQ_TIER_DIR"))
        try:
            backlog = None
            for name, kw in (("unbounded", None), ("equal_share", {}), ("fill", {"fill": True})):
                if kw is not None:
                    kw["spill_bytes"] = out["spill_bytes"]
                log = T.DurableLog(eng, os.path.join(root, name), parts, 0, start=starts, **(kw or {}))
                t0 = time.perf_counter()
                moved = log.spill()
                dt = time.perf_counter() - t0
                log.close()
                size = sum(int(f.pos[-1]) for f in log.parts.values())
                if backlog is None:
                    backlog = size
                    out.update(backlog_bytes=size, records=moved, spill_bytes=(size // 8) & ~15)
                assert size == backlog
                out[name] = {"seconds": round(dt, 4), "passes": log.passes or 1}
                shutil.rmtree(os.path.join(root, name))
        finally:
            shutil.rmtree(root, ignore_errors=True)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--spill", action="store_true")
    ap.add_argument("--spill-batches", type=int, default=4)
    ap.add_argument("--no-fetch", action="store_true", help="only the spill")
    args = ap.parse_args()
    spec = CONFIGS["B"]
    out = {"tool": "fetch_fill_probe", "config": "B", "requests": spec.partitions * 4, "replay": REPLAY}
    if not args.no_fetch:
        out.update(fetch_cost(args, spec, 4))
    if args.spill:
        out["spill"] = spill_cost(args, spec)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
