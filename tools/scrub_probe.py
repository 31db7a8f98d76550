"""Probe of rmq_scrub and of the verified fetch at BASELINE config B's shape (4,096 partitions, Zipf
1.1, 100 B, RF 3): fills an engine until the hot rings have wrapped, scrubs every partition under
rmq_profile_enable (kernel 2: an event before the plan kernel to one after the verify kernel), and
prints ONE JSON line: bytes scanned, records, kernel-2 ms, GB/s and the fraction of the HBM peak
bench.py uses; then the fetch kernels' region (kernel 4) at max = 10 and max = 1024 with and
without RMQ_FETCH_VERIFY.

    python tools/scrub_probe.py [--batches 192] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ripplemq_amd import _abi as A  # noqa: E402
from ripplemq_amd.engine import Engine, EngineConfig  # noqa: E402
from ripplemq_amd.workload import CONFIGS, make_batch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak: the constant of bench.py


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=192)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    spec = CONFIGS["B"]
    P, RF, S = spec.partitions, 3, 1 << 20
    cfg = EngineConfig(num_partitions=P, replication_factor=RF, segment_bytes=S, index_interval=1024,
                       max_batch_records=spec.records, max_batch_bytes=16 << 20, pipeline_depth=4, max_consumers=4)
    pool = [make_batch(spec, q) for q in range(8)]
    with Engine(cfg) as eng:
        for q in range(args.batches):
            b = pool[q % len(pool)]
            eng.append_async(b.pidx, b.lens, b.payload)
        eng.sync()
        st = eng.states()
        retained = int((st["log_end_pos"] - st["log_start_pos"]).sum())
        wrapped = int((st["log_end_pos"] > S).sum())
        ms = []
        for _ in range(args.reps + 1):  # the first run loads the kernels: dropped
            eng.profile(1)
            rows = eng.scrub()
            n, t = eng.profile_query(2)
            eng.profile(0)
            assert n == 1 and eng.last_scrub_rc == A.RMQ_OK and (rows["status"] == 0).all()
            ms.append(t)
        ms = sorted(ms[1:])
        med = ms[len(ms) // 2]
        scanned = int(rows["bytes_ok"].sum())
        assert scanned == RF * retained, (scanned, retained)
        line = {"tool": "scrub_probe", "config": "B", "partitions": P, "rf": RF, "segment_bytes": S,
                "batches": args.batches, "partitions_wrapped": wrapped,
                "bytes_scanned": scanned, "records": int(rows["records_ok"].sum()),
                "kernel2_ms": {"median": med, "min": ms[0], "max": ms[-1], "reps": len(ms)},
                "gbs": scanned / (med * 1e-3) / 1e9, "hbm_peak_gbs": HBM_PEAK_GBS,
                "hbm_frac": scanned / (med * 1e-3) / 1e9 / HBM_PEAK_GBS}
        # the fetch kernels with and without the flag: every consumer at its log start
        pp = np.repeat(np.arange(P, dtype=np.uint32), 4)
        cc = np.tile(np.arange(4, dtype=np.uint32), P)
        eng.commit_consumer_offset(pp, cc, np.repeat(st["log_start_offset"], 4))
        fetch = {}
        for mx in (10, 1024):
            cap = int(min(retained * 4, P * 4 * mx * 128)) + 4096
            d_out = eng.device_alloc(cap)
            req, res = eng.fetch_rows(P * 4)
            for verify in (False, True):
                req[:, 0], req[:, 1], req[:, 2], req[:, 3] = pp, cc, mx, (A.RMQ_FETCH_VERIFY if verify else 0)
                ts = []
                for _ in range(args.reps + 1):
                    eng.profile(1)
                    rc, r, used = eng.fetch_device(None, None, None, d_out, cap, req=req, res=res, pinned_rows=True)
                    n, t = eng.profile_query(4)
                    eng.profile(0)
                    assert rc == A.RMQ_OK and n == 1 and (r["status"] == 0).all()
                    ts.append(t * 1e3)
                ts = sorted(ts[1:])
                fetch[f"max{mx}_{'verify' if verify else 'plain'}_us"] = ts[len(ts) // 2]
            fetch[f"max{mx}_records"] = int(res["count"].sum())
            fetch[f"max{mx}_bytes"] = int(res["bytes"].sum())
            eng.device_free(d_out)
        line["fetch_kernel4"] = fetch
        print(json.dumps(line))


if __name__ == "__main__":
    main()
