"""The log states of tests/test_gpu_audit_sweep.py, built on the CPU oracle: each has the properties
the GPU tests rest on (no state can go vacuous silently), and the host walk refuses every flip of
the every-byte sweep at the flipped record, which is what lets the GPU tests demand that the scrub
and the verified fetch catch every one of them."""
import numpy as np
import pytest

import scrub_util as U
from parity import ring_window


@pytest.fixture(scope="module")
def ora3(oracle_mod):
    cfg = U.cfg3()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill3(e)  # (asserts that every record of every batch is appended)
        yield e, cfg


def test_state3_length_edges(ora3):
    e, cfg = ora3
    S = cfg.segment_bytes
    assert len(U.LENS3) == 89 and set(range(49)) <= set(U.LENS3) and {1023, 1024, 1025, 4095, 4096, 4097, 16384} <= set(U.BIG3)
    straddle = []
    for p in range(cfg.num_partitions):
        for r in range(cfg.replication_factor):
            k, bad, recs, st = U.host_walk(e, cfg, r, p)
            assert bad == U.NONE and k == st["log_end_offset"] - st["log_start_offset"], (p, r, bad)
        assert st["log_end_offset"] == U.BATCHES3 * len(U.LENS3)
        assert st["log_start_offset"] > 0 and st["log_end_pos"] > S, st  # wrapped
        assert len(recs) > 128, (p, len(recs))
        # the first 256 records (one consumer each in the one-record slices) hold every large length
        assert set(U.BIG3) <= {ln for _, _, ln in recs[:256]}, p
        assert {ln for _, _, ln in recs} == set(U.LENS3), p
        straddle += [ln for _, pos, ln in recs if ln > 1024 and (pos % S) + 16 + ln > S]
    assert straddle, "a record over 1024 B lies across the ring end"


def test_state4_many_partitions(oracle_mod):
    cfg = U.cfg4()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill4(e)
        s = e.states()
        for p in (0, 1024, 2499):
            assert U.host_walk(e, cfg, 1, p)[1] == U.NONE
    n = (s["log_end_offset"] - s["log_start_offset"]).astype(np.int64)
    assert len(n) == 2500 > 2 * 1024 and np.array_equal(n, U.counts4()) and not s["log_start_offset"].any()
    empty, few, many = int((n == 0).sum()), int(((n >= 1) & (n <= 3)).sum()), int(((n >= 10) & (n <= 25)).sum())
    assert empty + few + many == 2500 and min(empty, few, many) >= 800, (empty, few, many)
    assert (n[list(U.MARKED4)] >= 5).all()
    # tasks per slot as the scrub tiles a log (FORMAT.md §10): the short logs are one or two segments
    # (many runs per wave), the long ones several
    I = cfg.index_interval
    seg = s["log_end_pos"] // I - (s["log_start_pos"] + I - 1) // I + 2
    assert (seg[(n >= 1) & (n <= 3)] <= 3).all() and (seg[n >= 10] >= 4).all()
    assert int(seg.sum()) * cfg.replication_factor > 64 * 64  # more than one wave's tasks per workgroup wave


def test_state1_tasks_exceed_one_workgroup_pass(oracle_mod):
    # RMQ_AUDIT_WGS=1 leaves the scrub one workgroup of 4 waves, 256 tasks a pass
    cfg = U.cfg1()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill1(e)
        assert U.scrub_tasks(e.states(), cfg) > 256


def test_state1_host_walk_refuses_every_sweep_flip(oracle_mod):
    cfg = U.cfg1()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill1(e)
        st = e.state(U.SWEEP_P)
        win = ring_window(e, cfg, 0, U.SWEEP_P, st)
    k, bad, recs, _ = U.walk_window(win, st)
    assert bad == U.NONE and len(recs) > len(U.LENS1) and 3000 < win.size <= cfg.segment_bytes
    flips = U.sweep_positions(recs)
    if U.SWEEP_STRIDE is None:
        assert [w for w, _, _ in flips] == list(range(win.size))  # every byte of the window
    missed = []
    for w, i, d in flips:
        win[w] ^= U.SWEEP_MASK
        got = U.walk_window(win, st)[1]
        win[w] ^= U.SWEEP_MASK
        if got != recs[i][0]:
            missed.append((w, i, d, got))
    assert not missed, missed[:10]
    assert U.walk_window(win, st)[1] == U.NONE


def test_crc_consistent_padding_is_refused_by_the_host_walk(oracle_mod):
    # the padding that only the zero-padding rule catches (tests/test_gpu_audit_sweep.py writes it
    # into a ring): the CRC over the padded pieces is the clean one, and the host walk still refuses
    cfg = U.cfg1()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill1(e)
        st = e.state(U.SWEEP_P)
        win = ring_window(e, cfg, 0, U.SWEEP_P, st)
    recs = U.walk_window(win, st)[2]
    for ln in (17, 241, 600):
        i, rec = next((i, x) for i, x in enumerate(recs) if x[2] == ln)
        a = rec[1] - recs[0][1] + 16
        pad = -ln % 16
        bad = U.crc_consistent_padding(win[a:a + ln].tobytes(), pad, oracle_mod.crc32c)
        assert len(bad) == pad and bad[0] and not win[a + ln:a + ln + pad].any()
        keep = win[a + ln:a + ln + pad].copy()
        win[a + ln:a + ln + pad] = np.frombuffer(bad, np.uint8)
        assert U.walk_window(win, st)[1] == rec[0]
        win[a + ln:a + ln + pad] = keep
    assert U.walk_window(win, st)[1] == U.NONE
