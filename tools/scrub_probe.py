"""Probe of rmq_scrub and of the verified fetch at BASELINE config B's shape (4,096 partitions, Zipf
1.1, 100 B, RF 3): fills an engine until the hot rings have wrapped, scrubs every partition under
rmq_profile_enable (kernel 2: an event before the plan kernel to one after the verify kernel), and
prints ONE JSON line: bytes scanned, records, kernel-2 ms, GB/s and the fraction of the HBM peak
bench.py uses; then the fetch kernels' region (kernel 4) at max = 10 and max = 1024 with and
without RMQ_FETCH_VERIFY. The repair leg (rmq_repair, kernel 5: an event before its first kernel to one
after its last) runs on the same state in the same process: on the clean logs, beside the scrub,
and after slot 1 of every tenth partition was damaged in every segment of its retained log (one
byte flipped per segment with rmq_fault_flip_ring, the first byte of the segment's first header),
so every segment of those slots is rewritten from slot 0.

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


def repair_leg(eng, cfg, st, reps, scrub_ms) -> dict:
    P, S, I = cfg.num_partitions, cfg.segment_bytes, cfg.index_interval
    ts = []
    for _ in range(reps + 1):  # clean logs: the first pass alone
        eng.profile(1)
        rows = eng.repair()
        n, t = eng.profile_query(5)
        eng.profile(0)
        assert n == 1 and eng.last_repair_rc == A.RMQ_OK and not rows["segments_repaired"].any()
        ts.append(t)
    ts = sorted(ts[1:])
    out = {"clean_kernel5_ms": {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "reps": len(ts)},
           "clean_minus_scrub_ms": ts[len(ts) // 2] - scrub_ms[len(scrub_ms) // 2],
           "scrub_spread_ms": scrub_ms[-1] - scrub_ms[0]}
    # slot 1 of every tenth partition: one flip at the start of every non-empty segment
    flips, nbytes = [], 0
    for p in range(0, P, 10):
        sp, ep = int(st["log_start_pos"][p]), int(st["log_end_pos"][p])
        lo, hi = (sp + I - 1) // I, ep // I
        cuts = [sp] + ([int(x) for x in eng.read_index(p, lo, hi - lo + 1)[:, 1]] if lo <= hi else []) + [ep]
        for a, b in zip(cuts, cuts[1:]):
            if b > a:
                flips.append((p, a % S))
                nbytes += b - a
    ts = []
    for _ in range(reps + 1):
        for p, off in flips:
            eng.fault_flip_ring(1, p, off)
        eng.profile(1)
        rows = eng.repair()
        n, t = eng.profile_query(5)
        eng.profile(0)
        assert n == 1 and eng.last_repair_rc == A.RMQ_OK and not rows["segments_unrepaired"].any()
        assert (int(rows["segments_repaired"].sum()), int(rows["bytes_repaired"].sum())) == (len(flips), nbytes)
        ts.append(t)
    ts = sorted(ts[1:])
    med = ts[len(ts) // 2]
    clean = out["clean_kernel5_ms"]["median"]
    out.update({"damaged_partitions": len(range(0, P, 10)), "segments_rewritten": len(flips), "bytes_rewritten": nbytes,
                "damaged_kernel5_ms": {"median": med, "min": ts[0], "max": ts[-1], "reps": len(ts)},
                # two audits (about twice the clean call) and the copy between them
                "rewrite_gbs_whole_call": nbytes / (med * 1e-3) / 1e9,
                "rewrite_gbs_copy_alone": nbytes / (max(med - 2 * clean, 1e-6) * 1e-3) / 1e9})
    assert eng.scrub() is not None and eng.last_scrub_rc == A.RMQ_OK
    return out


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
        line["repair"] = repair_leg(eng, cfg, st, args.reps, ms)
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
