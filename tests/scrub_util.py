"""Shared by tests/test_gpu_scrub.py and tests/test_gpu_fetch_verify.py: the two log states the
issue names, the host walk that gives every expected value (rmq_scan_records with RMQ_SCAN_CHECK
over the retained bytes read back with read_segment; host code pinned by tests/test_tier.py), and
the record map used to choose flip positions. Works on the GPU engine and on the oracle alike
(both expose append / state / read_segment), so the shapes are checked on the CPU too.
"""
from __future__ import annotations

import numpy as np

from parity import ring_window
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import EngineConfig
from ripplemq_amd.tier import _scan

NONE = A.RMQ_OFFSET_NONE

# state 1: an empty payload, no padding, a record ending exactly on an interval, records spanning 2
# and 6 intervals (repeated index entries)
LENS1 = (0, 1, 15, 16, 17, 100, 239, 240, 241, 600, 1500)
ACTIVE1 = 6          # partitions 0..5 take the cycles; 6 stays empty; 7 holds one 16-byte record
BATCHES1 = 4
# state 2: above the whole-wave threshold (64 pieces), one record wraps the ring end
LENS2 = (1008, 1040, 5000, 9000)


def cfg1(**kw) -> EngineConfig:
    d = dict(num_partitions=8, replication_factor=3, segment_bytes=4096, index_interval=256, max_consumers=4,
             max_batch_records=256, max_batch_bytes=1 << 16)
    d.update(kw)
    return EngineConfig(**d)


def cfg2() -> EngineConfig:
    return EngineConfig(num_partitions=8, replication_factor=3, segment_bytes=16384, index_interval=1024,
                        max_consumers=4, max_batch_records=64, max_batch_bytes=1 << 16)


def batch1(b: int):
    """One cycle of LENS1 per active partition, rotated per partition and batch, interleaved:
    3,216 record bytes per partition, under segment - interval."""
    rng = np.random.default_rng(1000 + b)
    pidx, lens = [], []
    for j in range(len(LENS1)):
        for p in range(ACTIVE1):
            pidx.append(p)
            lens.append(LENS1[(j + p + b) % len(LENS1)])
    payload = rng.integers(0, 256, sum(lens), dtype=np.uint8)
    return np.array(pidx, np.uint32), np.array(lens, np.uint32), payload


def fill1(eng, batches: int = BATCHES1) -> None:
    eng.append(np.array([7], np.uint32), np.array([0], np.uint32), np.zeros(0, np.uint8))
    for b in range(batches):
        _, st = eng.append(*batch1(b))
        assert st["appended"] == ACTIVE1 * len(LENS1), st


def batch2(b: int):
    rng = np.random.default_rng(2000 + b)
    pidx, lens = [], []
    for p in range(4):  # one large record per partition and batch, a different one each time
        pidx.append(p)
        lens.append(LENS2[(p + b) % len(LENS2)])
    payload = rng.integers(0, 256, sum(lens), dtype=np.uint8)
    return np.array(pidx, np.uint32), np.array(lens, np.uint32), payload


def fill2(eng, batches: int = 8) -> None:
    for b in range(batches):
        _, st = eng.append(*batch2(b))
        assert st["appended"] == 4, st


def host_walk(eng, cfg, replica: int, p: int):
    """The host walk of one replica's retained log: (records accepted, first bad offset or NONE,
    [(offset, logical position, payload length)] of the accepted records, state)."""
    st = eng.state(p)
    buf = ring_window(eng, cfg, replica, p, st)
    want = st["log_end_offset"] - st["log_start_offset"]
    k, nb, pos = _scan(buf, st["log_start_offset"], want, True, True)
    recs = []
    for i in range(k):
        ln = int.from_bytes(buf[pos[i] + 8:pos[i] + 12].tobytes(), "little")
        recs.append((st["log_start_offset"] + i, st["log_start_pos"] + int(pos[i]), ln))
    clean = k == want and nb == buf.size
    return k, (NONE if clean else st["log_start_offset"] + k), recs, st


def clean_totals(eng, cfg):
    """Per partition (records, bytes) of one replica's retained log, from the engine state."""
    out = []
    for p in range(cfg.num_partitions):
        st = eng.state(p)
        out.append((st["log_end_offset"] - st["log_start_offset"], st["log_end_pos"] - st["log_start_pos"]))
    return out


def assert_clean(rows, eng, cfg, replicas: int | None = None) -> None:
    rf = cfg.replication_factor if replicas is None else replicas
    for p, (n, nb) in enumerate(clean_totals(eng, cfg)):
        r = rows[p]
        assert int(r["status"]) == A.RMQ_OK and int(r["bad_offset"]) == NONE, (p, r)
        assert (int(r["replicas"]), int(r["records_ok"]), int(r["bytes_ok"])) == (rf, rf * n, rf * nb), (p, r, n, nb)
