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


# state 3, "length edges": every length 0..48, then the lengths around each piece count at which a
# kernel takes another path (112 B: the apply stage's LDS image; 1024 B = 64 pieces: the whole-wave
# threshold of the scrub, the fetch verify and the ingest; 4096 B = 256 pieces: one or two rounds of
# wave_crc_pieces; multiples of 64 pieces and their neighbours)
LENS3 = tuple(range(49)) + (111, 112, 113, 127, 128, 129, 239, 240, 241, 255, 256, 257, 1007, 1008, 1009,
                            1023, 1024, 1025, 1039, 1040, 1041, 2047, 2048, 2049, 4079, 4080, 4081,
                            4095, 4096, 4097, 4111, 4112, 8191, 8192, 8193, 12287, 12288, 12289, 16383, 16384)
PARTS3 = 4
# One cycle is about 148 KB of records per partition. Two cycles in a 256 KiB ring retain the second
# and the 12 to 15 largest records of the first, 101 to 104 records in all, so the rings are
# 512 KiB and take four cycles: 273 to 276 records stay.
BATCHES3 = 4
BIG3 = tuple(x for x in LENS3 if x >= 1023)
# state 4, "many partitions": two full chunks of the scrub plan's 1024 partitions and a partial one
P4 = 2500
MARKED4 = (0, 63, 64, 1023, 1024, 2047, 2048, 2499)  # wave, chunk and range edges: at least 5 records each


def cfg3() -> EngineConfig:
    return EngineConfig(num_partitions=PARTS3, replication_factor=2, segment_bytes=1 << 19, index_interval=1024,
                        max_consumers=256, max_batch_records=1024, max_batch_bytes=1 << 20)


def batch3(b: int):
    """One cycle of LENS3 per partition, rotated per partition and batch, interleaved (as batch1)."""
    rng = np.random.default_rng(3000 + b)
    pidx, lens = [], []
    for j in range(len(LENS3)):
        for p in range(PARTS3):
            pidx.append(p)
            lens.append(LENS3[(j + p + b) % len(LENS3)])
    payload = rng.integers(0, 256, sum(lens), dtype=np.uint8)
    return np.array(pidx, np.uint32), np.array(lens, np.uint32), payload


def fill3(eng) -> None:
    for b in range(BATCHES3):
        _, st = eng.append(*batch3(b))
        assert st["appended"] == PARTS3 * len(LENS3), st


def cfg4() -> EngineConfig:
    return EngineConfig(num_partitions=P4, replication_factor=2, segment_bytes=4096, index_interval=256,
                        max_consumers=2, max_batch_records=1 << 16, max_batch_bytes=1 << 22)


def counts4() -> np.ndarray:
    """Records per partition of state 4: by p mod 3 none, one to three, or 10 to 25 (at most
    25 * 144 = 3,600 record bytes, under segment - interval); the marked partitions 10 to 25."""
    p = np.arange(P4)
    n = np.where(p % 3 == 0, 0, np.where(p % 3 == 1, 1 + (p // 3) % 3, 10 + (7 * p) % 16))
    n[list(MARKED4)] = 10 + (7 * np.array(MARKED4)) % 16
    return n


def batch4():
    rng = np.random.default_rng(4000)
    pidx = rng.permutation(np.repeat(np.arange(P4), counts4())).astype(np.uint32)
    lens = rng.integers(0, 121, pidx.size).astype(np.uint32)
    payload = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    return pidx, lens, payload


def fill4(eng) -> None:
    b = batch4()
    _, st = eng.append(*b)
    assert st["appended"] == b[0].size, st


# Every byte of one retained log (state 1, partition SWEEP_P) is flipped with SWEEP_MASK, on
# SWEEP_SCRUB_SLOT for the scrub and on slot 0 (the one the gather reads) for the fetch.
SWEEP_P, SWEEP_MASK, SWEEP_SCRUB_SLOT = 3, 0x5A, 2
SWEEP_STRIDE = None  # None: every payload byte; k (coprime to 16): see sweep_positions


def sweep_positions(recs, stride=SWEEP_STRIDE):
    """[(window byte, record index, byte of the record)] of the flips of the every-byte sweep over
    the record map `recs` of a clean log: every byte of the window, or with a stride every header
    byte, every padding byte, the first, middle and last payload byte of each record and every
    stride-th window byte of the rest. tests/test_audit_states.py checks this very list on the CPU."""
    out = []
    base = recs[0][1]
    for i, (_, pos, ln) in enumerate(recs):
        rs = 16 + ((ln + 15) & ~15)
        for d in range(rs):
            w = pos - base + d
            pay = 16 <= d < 16 + ln
            if stride is None or not pay or d - 16 in (0, ln // 2, ln - 1) or w % stride == 0:
                out.append((w, i, d))
    return out


def crc_consistent_padding(payload: bytes, pad: int, crc32c) -> bytes:
    """`pad` (8..15) padding bytes, the first of them non-zero, that leave the CRC32C register where
    zero padding leaves it: crc32c(payload + result) == crc32c(payload + bytes(pad)). A check that
    runs the CRC over a record's zero-padded pieces passes such a record; only the zero-padding rule
    itself (FORMAT.md §1) refuses it. crc32c(A + D) is affine in the four bytes D over GF(2), so D
    is found by elimination over its 32 bits."""
    assert 8 <= pad <= 15
    head = payload + b"\x01\x00\x00\x00"
    c0 = crc32c(head + bytes(4))
    basis = {}  # leading bit -> (vector, the bits of D that give it)
    for i in range(32):
        v, comb = crc32c(head + (1 << i).to_bytes(4, "little")) ^ c0, 1 << i
        while v:
            h = v.bit_length() - 1
            if h not in basis:
                basis[h] = (v, comb)
                break
            v, comb = v ^ basis[h][0], comb ^ basis[h][1]
    t, d = crc32c(payload + bytes(8)) ^ c0, 0
    while t:
        bv, bc = basis[t.bit_length() - 1]
        t, d = t ^ bv, d ^ bc
    out = b"\x01\x00\x00\x00" + d.to_bytes(4, "little") + bytes(pad - 8)
    assert crc32c(payload + out) == crc32c(payload + bytes(pad))
    return out


def scrub_tasks(states, cfg) -> int:
    """(replica slot, segment) pairs of a scrub over these partition states (FORMAT.md §10: the live
    index entries lo..hi tile a log into hi - lo + 2 segments, one without a live entry)."""
    I = cfg.index_interval
    lo = (states["log_start_pos"].astype(np.int64) + I - 1) // I
    hi = states["log_end_pos"].astype(np.int64) // I
    return int(np.where(lo <= hi, hi - lo + 2, 1).sum()) * cfg.replication_factor


def assert_clean_bulk(rows, states, rf: int) -> None:
    """assert_clean for many partitions: `states` is Engine.states() of the rows' partitions."""
    n = (states["log_end_offset"] - states["log_start_offset"]).astype(np.uint64)
    nb = (states["log_end_pos"] - states["log_start_pos"]).astype(np.uint64)
    assert len(rows) == len(states)
    bad = np.flatnonzero((rows["status"] != A.RMQ_OK) | (rows["bad_offset"] != NONE) | (rows["replicas"] != rf) |
                         (rows["records_ok"] != rf * n) | (rows["bytes_ok"] != rf * nb))
    assert bad.size == 0, (bad[:8], rows[bad[:8]], n[bad[:8]], nb[bad[:8]])


def walk_window(buf, st):
    """host_walk of bytes already read back: `buf` is the retained window of a log in state `st`."""
    want = st["log_end_offset"] - st["log_start_offset"]
    k, nb, pos = _scan(buf, st["log_start_offset"], want, True, True)
    recs = []
    for i in range(k):
        ln = int.from_bytes(buf[pos[i] + 8:pos[i] + 12].tobytes(), "little")
        recs.append((st["log_start_offset"] + i, st["log_start_pos"] + int(pos[i]), ln))
    clean = k == want and nb == buf.size
    return k, (NONE if clean else st["log_start_offset"] + k), recs, st


def host_walk(eng, cfg, replica: int, p: int):
    """The host walk of one replica's retained log: (records accepted, first bad offset or NONE,
    [(offset, logical position, payload length)] of the accepted records, state)."""
    st = eng.state(p)
    return walk_window(ring_window(eng, cfg, replica, p, st), st)


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
