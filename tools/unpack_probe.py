"""Cost of rmq_unpack beside the fetch that made its input (FORMAT.md §7 "Record columns").

Shapes: BASELINE config B (4,096 partitions, Zipf 1.1, 100 B, RF 3, rings of 1 MiB; 4 consumers per
partition lagging the high watermark by U[0, retained records], as bench.py's fetch leg), one table
fetch over the 16,384 (partition, consumer) rows at max = 10 and at max = 1024; and config D's records
(log-uniform 64 B to 16 KiB), 4,096 rows reading everything retained. Rows, output, table and columns
all in device memory.

Per shape: the resolve-plus-gather region of the fetch (rmq_profile_query kernel 4, the yardstick:
existing code, same run) and its table kernels (kernel 9); then per mode (view, packed, stride 128)
the span of rmq_unpack (kernel 11: an event before its first kernel to one after its last), --reps
times, with the bytes the call must move (headers and table words read, columns written, payload
bytes read as 16-byte pieces and written) as a fraction of bench.py's HBM peak; and once the wall time
of table_records on the same output copied to the host, the decode the call replaces. ONE JSON line
per shape reports medians with min-max.

    python tools/unpack_probe.py [--reps 10] [--shapes B10,B1024,D]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import HBM_PEAK_GBS  # noqa: E402
from ripplemq_amd import _abi as A  # noqa: E402
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, EngineConfig, table_records  # noqa: E402
from ripplemq_amd.workload import CONFIGS, make_batch  # noqa: E402

STRIDE = 128


def stat(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3), "reps": len(ts)}


def engine_for(config: str):
    """(engine, pidx, consumer) of a shape's rows, the log filled and the consumers placed."""
    spec = CONFIGS[config]
    P = spec.partitions
    if config == "B":
        NC, batches = 4, 48
        cfg = EngineConfig(num_partitions=P, replication_factor=3, segment_bytes=1 << 20, index_interval=1024,
                           max_batch_records=spec.records, max_batch_bytes=16 << 20, pipeline_depth=4, max_consumers=NC)
    else:
        NC, batches = 1, 16
        cfg = EngineConfig(num_partitions=P, replication_factor=3, segment_bytes=1 << 20, index_interval=1024,
                           max_batch_records=spec.records, max_batch_bytes=64 << 20, pipeline_depth=4, max_consumers=4)
    eng = Engine(cfg)
    pool = [make_batch(spec, q) for q in range(8)]
    for q in range(batches):
        b = pool[q % len(pool)]
        eng.append(b.pidx, b.lens, b.payload)
    pp, cc = np.repeat(np.arange(P, dtype=np.uint32), NC), np.tile(np.arange(NC, dtype=np.uint32), P)
    st = eng.states()
    hw, lo = st["high_watermark"].astype(np.int64), st["log_start_offset"].astype(np.int64)
    if config == "B":
        g = np.random.default_rng(0x52495050)
        behind = (g.random(P * NC) * (np.repeat(hw - lo, NC) + 1)).astype(np.int64)
        eng.commit_consumer_offset(pp, cc, (np.repeat(hw, NC) - behind).astype(np.uint64))
    else:
        eng.commit_consumer_offset(pp, cc, lo.astype(np.uint64))
    eng.sync()
    return eng, pp, cc


def probe(eng, pp, cc, mx: int, reps: int, name: str) -> dict:
    n = len(pp)
    req = np.zeros((n, 4), np.uint32)
    req[:, 0], req[:, 1], req[:, 2] = pp, cc, mx
    held = []

    def dev(nbytes, src=None):
        p = eng.device_alloc(max(int(nbytes), 16))
        held.append(p)
        if src is not None:
            eng.h2d(p, src)
        return p

    d_req, d_res = dev(16 * n, req.view(np.uint8).reshape(-1)), dev(32 * n)
    _, _, cap = eng.fetch_device(None, None, None, 0, 0, d_rows=(n, d_req, d_res))  # bytes needed
    words = cap // 16 + n
    d_out, d_row, d_pos, d_first = dev(cap), dev(8 * (n + 1)), dev(8 * words), dev(8 * (n + 1))
    out = {"tool": "unpack_probe", "shape": name, "rows": n, "max_records": mx, "fetch_bytes": int(cap)}
    reg4, reg9 = [], []
    for k in range(reps + 1):
        eng.profile(1)
        rc, _, used = eng.fetch_device(None, None, None, d_out, cap, d_rows=(n, d_req, d_res), table=(d_row, d_pos, words))[:3]
        runs, ms4 = eng.profile_query(4)
        _, ms9 = eng.profile_query(9)
        eng.profile(0)
        assert rc == 0 and used == cap and runs == 1
        if k:
            reg4.append(ms4 * 1e3), reg9.append(ms9 * 1e3)
    out["fetch_region4_us"], out["fetch_table_region9_us"] = stat(reg4), stat(reg9)
    common = dict(buf=d_out, buf_bytes=cap, rows=d_res, n=n, rec_row=d_row, rec_pos=d_pos, rec_words=words, rec_first=d_first)
    size = eng.unpack_device(**common, payload=d_out)  # the packed size probe
    R, packed = size["records"], size["payload_bytes"]
    out["records"], out["payload_bytes"] = R, packed
    d_off, d_len, d_poff, d_tag = dev(8 * R), dev(4 * R), dev(8 * R), dev(4 * R)
    d_pay = dev(max(packed, R * STRIDE))
    cols = dict(offset=d_off, len=d_len, payload_off=d_poff, tag=d_tag, rec_cap=R)
    lens = None
    for mode, kw in (("view", {}), ("packed", dict(payload=d_pay, payload_cap=packed)),
                     (f"stride{STRIDE}", dict(payload=d_pay, payload_cap=R * STRIDE, stride=STRIDE))):
        spans = []
        for k in range(reps + 1):
            eng.profile(1)
            res = eng.unpack_device(**common, **cols, **kw)
            calls, ms = eng.profile_query(11)
            eng.profile(0)
            assert res["status"] == A.RMQ_OK and res["records"] == R and calls == 1 and not res["mismatched"]
            if k:
                spans.append(ms * 1e3)
        if lens is None:
            lens = np.empty(R, np.uint32)
            eng.d2h(lens, d_len)
            assert int(lens.sum(dtype=np.uint64)) == packed
        # headers and table words read twice (the records pass and the emit pass), columns written once
        moved = R * (2 * 16 + 2 * 8 + 8 + 4 + 8 + 4)
        if mode == "packed":
            moved += int(((lens.astype(np.uint64) + 15) & ~np.uint64(15)).sum()) + packed
        elif mode != "view":
            moved += int(((np.minimum(lens, STRIDE).astype(np.uint64) + 15) & ~np.uint64(15)).sum()) + R * STRIDE
        s = stat(spans)
        out[f"unpack_{mode}_us"] = s
        out[f"unpack_{mode}_bytes_moved"] = int(moved)
        out[f"unpack_{mode}_hbm_fraction"] = round(moved / (s["median"] * 1e-6) / (HBM_PEAK_GBS * 1e9), 4)
        out[f"unpack_{mode}_over_fetch"] = round(s["median"] / out["fetch_region4_us"]["median"], 3)
    # the host decode the call replaces, on the same output
    buf, res, row, pos = np.empty(cap, np.uint8), np.zeros(n, FETCH_RES_DTYPE), np.empty(n + 1, np.uint64), np.empty(words, np.uint64)
    eng.d2h(buf, d_out), eng.d2h(res.view(np.uint8), d_res), eng.d2h(row.view(np.uint8), d_row), eng.d2h(pos.view(np.uint8), d_pos)
    t0 = time.perf_counter()
    recs = table_records(buf, res, row, pos)
    out["host_table_records_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    assert sum(len(x) for x in recs) == R
    for p in held:
        eng.device_free(p)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="B10,B1024,D")
    args = ap.parse_args()
    shapes = args.shapes.split(",")
    for config in ("B", "D"):
        todo = [s for s in shapes if s.startswith(config)]
        if not todo:
            continue
        eng, pp, cc = engine_for(config)
        with eng:
            for s in todo:
                mx = int(s[1:]) if len(s) > 1 else 1 << 20
                print(json.dumps(probe(eng, pp, cc, mx, args.reps, s)), flush=True)


if __name__ == "__main__":
    main()
