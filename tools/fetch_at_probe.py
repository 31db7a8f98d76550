"""Cost of explicit offsets (rmq_fetch_at) at BASELINE config B's shape (4,096 partitions, Zipf 1.1,
100 B, RF 3, rings of 1 MiB; 4 consumers per partition lagging the high watermark by
U[0, retained records], as bench.py's fetch leg): one fetch of the 16,384 requests at max = 10 and
at max = 1024, as rmq_fetch from the committed offsets ("plain") and as rmq_fetch_at with those same
offsets passed explicitly ("at"), so both serve the same slices and bytes (rows, offsets and output
in device memory). Each is timed by the engine's own fetch profile (rmq_profile_query kernel 4: an
event before the ticket's first kernel to one after its last), replayed eight times back to back
(per run), --reps times, alternating, and ONE JSON line reports the medians with min-max.

--mode plain uses only calls that exist without rmq_fetch_at, so the same file measures a tree
that lacks it: the yardstick.

    python tools/fetch_at_probe.py [--batches 48] [--reps 20] [--mode both|plain]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, EngineConfig  # noqa: E402
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
        offs = (np.repeat(hw, NC) - lag).astype(np.uint64)
        eng.commit_consumer_offset(pp, cc, offs)
        eng.sync()
        d_req, d_res, d_at = (eng.device_alloc(x) for x in (16 * n, 32 * n, 8 * n))
        eng.h2d(d_at, offs.view(np.uint8))
        out = {"tool": "fetch_at_probe", "config": "B", "requests": n, "mode": args.mode, "replay": REPLAY}
        for mx in (10, 1024):
            req = np.zeros((n, 4), np.uint32)
            req[:, 0], req[:, 1], req[:, 2] = pp, cc, mx
            eng.h2d(d_req, req.view(np.uint8).reshape(-1))
            _, _, cap = eng.fetch_device(None, None, None, 0, 0, d_rows=(n, d_req, d_res))  # bytes needed
            d_out = eng.device_alloc(cap)
            res = {}

            def timed(at):
                eng.profile(REPLAY)
                kw = {"offsets": d_at} if at else {}
                rc, _, used = eng.fetch_device(None, None, None, d_out, cap, d_rows=(n, d_req, d_res), **kw)
                runs, ms = eng.profile_query(4)
                eng.profile(0)
                assert rc == 0 and runs == REPLAY and used == cap, (rc, runs, used, cap)
                rows = np.empty(n, FETCH_RES_DTYPE)
                eng.d2h(rows.view(np.uint8), d_res)
                res[at] = rows
                return ms * 1e3 / runs

            modes = (False, True) if args.mode == "both" else (False,)
            ts = {m: [] for m in modes}
            for m in modes:  # warm-up: code objects, slots
                timed(m)
            for _ in range(args.reps):
                for m in modes:
                    ts[m].append(timed(m))
            if args.mode == "both":
                assert np.array_equal(res[False], res[True])  # the same slices and bytes
            leg = {"bytes": int(cap), "records": int(res[False]["count"].sum()), "plain_us": stat(ts[False])}
            if args.mode == "both":
                leg["at_us"] = stat(ts[True])
                leg["at_minus_plain_us"] = round(leg["at_us"]["median"] - leg["plain_us"]["median"], 3)
            out[f"max{mx}"] = leg
            eng.device_free(d_out)
        print(json.dumps(out))


if __name__ == "__main__":
    main()
