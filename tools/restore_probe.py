"""Probe of the restart paths at BASELINE config B's shape (4,096 partitions, Zipf 1.1, 100 B, RF 3,
rings of 1 MiB): an engine takes batches with a DurableLog.spill after each one (files from offset
0), then tier.restore and tier.replay load fresh engines from those files in the same process,
alternating, and ONE JSON line reports the wall time of each (median of --reps after a warm-up pair,
with min-max), their ratio, where restore's wall time goes (opening the files, reading the runs,
the rmq_restore calls, the consumer rows and terms), and rmq_profile_query kernel 7's region (an
event before the verify kernel to one after the finish kernel, per call) with the bytes installed
over it as a fraction of the HBM peak bench.py uses.

    python tools/restore_probe.py [--batches 64] [--reps 5] [--dir DIR]
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
from ripplemq_amd.engine import Engine, EngineConfig  # noqa: E402
from ripplemq_amd.workload import CONFIGS, make_batch  # noqa: E402

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak: the constant of bench.py
CURSOR = 3
REPLAY_BATCH = 8000    # replay's last batches hold one hot partition's records: under its ring less an interval


def stat(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1], "reps": len(ts)}


def timed_restore(cfg, root, P, dry=False):
    """tier.restore into a fresh engine: wall seconds, its phases, kernel 7 and what it installed.
    dry: every rmq_restore call with RMQ_RESTORE_DRY_RUN (kernel 7 is then the verify kernel alone)."""
    phases = {}
    real = {k: getattr(T._PartitionFiles, k) for k in ("__init__", "read_bytes")}

    def wrap(name, key):
        fn = real[name]

        def inner(*a, **kw):
            t = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                phases[key] = phases.get(key, 0.0) + time.perf_counter() - t
        return inner

    with Engine(cfg) as eng:
        call = eng.restore

        def restore_call(*a, **kw):
            t = time.perf_counter()
            try:
                return call(*a, dry_run=dry, **kw)
            finally:
                phases["rmq_restore_s"] = phases.get("rmq_restore_s", 0.0) + time.perf_counter() - t
                phases["calls"] = phases.get("calls", 0) + 1

        eng.restore = restore_call
        T._PartitionFiles.__init__ = wrap("__init__", "open_files_s")
        T._PartitionFiles.read_bytes = wrap("read_bytes", "read_runs_s")
        try:
            eng.profile(1)
            t0 = time.perf_counter()
            out = T.restore(root, eng, range(P))
            wall = time.perf_counter() - t0
        finally:
            T._PartitionFiles.__init__ = real["__init__"]
            T._PartitionFiles.read_bytes = real["read_bytes"]
        calls, ms = eng.profile_query(7)
        eng.profile(0)
        if dry:
            return wall, phases, calls, ms, 0, out
        st = eng.states()
        nbytes = int((st["log_end_pos"] - st["log_start_pos"]).sum())
        assert calls == phases["calls"] and int((st["log_end_offset"] - st["log_start_offset"]).sum()) == out["records"]
        rows = eng.scrub()
        assert eng.last_scrub_rc == 0 and int(rows["bytes_ok"].sum()) == cfg.replication_factor * nbytes
    phases["rest_s"] = wall - sum(v for k, v in phases.items() if k.endswith("_s"))
    return wall, phases, calls, ms, nbytes, out


def timed_replay(cfg, root, P):
    with Engine(cfg) as eng:
        t0 = time.perf_counter()
        out = T.replay(root, eng, range(P), batch_records=REPLAY_BATCH)
        return time.perf_counter() - t0, out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the segment files go (default: a temporary folder)")
    args = ap.parse_args()
    spec = CONFIGS["B"]
    P, RF, S = spec.partitions, 3, 1 << 20
    cfg = EngineConfig(num_partitions=P, replication_factor=RF, segment_bytes=S, index_interval=1024,
                       max_batch_records=spec.records, max_batch_bytes=16 << 20, pipeline_depth=4, max_consumers=4)
    root = tempfile.mkdtemp(prefix="restore_probe_", dir=args.dir)
    try:
        pool = [make_batch(spec, q) for q in range(8)]
        t0 = time.perf_counter()
        with Engine(cfg) as eng:
            log = T.DurableLog(eng, root, range(P), CURSOR)
            for q in range(args.batches):  # the second hottest partition takes 0.6 MiB a batch: spill after each
                b = pool[q % len(pool)]
                eng.append(b.pidx, b.lens, b.payload)
                log.spill()
            log.close()
            st = eng.states()
        fill_s = time.perf_counter() - t0
        durable = int(st["log_end_offset"].sum())
        file_bytes = int(st["log_end_pos"].sum())
        wrapped = int((st["log_end_pos"] > S).sum())
        rs, rp, k7, k7dry, phases = [], [], [], [], []
        for rep in range(args.reps + 1):  # the first pair loads the kernels and warms the page cache: dropped
            w, ph, calls, ms, nbytes, ro = timed_restore(cfg, root, P)
            wr, po = timed_replay(cfg, root, P)
            assert po["records"] == durable and ro["partitions"] == po["partitions"]
            dry_ms = timed_restore(cfg, root, P, dry=True)[3]
            if rep:
                rs.append(w), rp.append(wr), k7.append(ms), phases.append(ph), k7dry.append(dry_ms)
            print(json.dumps({"rep": rep, "restore_s": w, "replay_s": wr, "kernel7_ms": ms, "calls": calls}), file=sys.stderr,
                  flush=True)
        med = stat(k7)["median"]
        mid = phases[int(np.argsort(rs)[len(rs) // 2])]
        line = {"tool": "restore_probe", "config": "B", "partitions": P, "rf": RF, "segment_bytes": S,
                "batches": args.batches, "partitions_wrapped": wrapped, "durable_records": durable,
                "file_bytes": file_bytes, "fill_and_spill_s": fill_s,
                "restored_records": ro["records"], "restored_bytes_per_replica": nbytes,
                "restore_wall_s": stat(rs), "replay_wall_s": stat(rp),
                "replay_over_restore": stat(rp)["median"] / stat(rs)["median"],
                "restore_phases_of_median_run": mid,
                "kernel7_ms_per_run": stat(k7), "kernel7_dry_run_ms_per_run": stat(k7dry), "kernel7_calls_per_run": calls, "kernel7_ms_per_call": med / calls,
                "read_gbs": nbytes / (med * 1e-3) / 1e9, "installed_gbs": RF * nbytes / (med * 1e-3) / 1e9,
                "moved_gbs": (2 + RF) * nbytes / (med * 1e-3) / 1e9,  # the run read twice, RF rings written
                "hbm_peak_gbs": HBM_PEAK_GBS, "installed_hbm_frac": RF * nbytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "moved_hbm_frac": (2 + RF) * nbytes / (med * 1e-3) / 1e9 / HBM_PEAK_GBS}
        print(json.dumps(line))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
