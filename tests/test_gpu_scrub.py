"""rmq_scrub on the GPU (FORMAT.md §10): clean logs of mixed and large records, every class of
flipped byte, range errors, after a ring move, after follower truncation and rebase. Every expected
value comes from the host walk (tests/scrub_util.py: rmq_scan_records over the bytes read back),
never from the scrub itself."""
import threading

import numpy as np
import pytest

import scrub_util as U
from repl_sim import leader_change_script, place, rank_cfg
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine, EngineConfig, EngineError, LocalHub
from ripplemq_amd.sharding import rank_view
from ripplemq_amd.workload import StreamSpec, make_batch

pytestmark = pytest.mark.gpu

CRC, CHAIN = A.RMQ_SCRUB_BAD_CRC, A.RMQ_SCRUB_BAD_CHAIN


@pytest.fixture(scope="module")
def state1():
    cfg = U.cfg1()
    with Engine(cfg) as e:
        U.fill1(e)
        yield e, cfg


@pytest.fixture(scope="module")
def state2():
    cfg = U.cfg2()
    with Engine(cfg) as e:
        U.fill2(e)
        yield e, cfg


def test_clean_mixed_sizes(state1):
    e, cfg = state1
    I = cfg.index_interval
    sts = [e.state(p) for p in range(cfg.num_partitions)]
    for p in range(U.ACTIVE1):  # wrapped at least twice, log start off a multiple of the interval
        assert sts[p]["log_end_pos"] >= 2 * cfg.segment_bytes and sts[p]["log_start_pos"] % I, sts[p]
    assert sts[6]["log_end_offset"] == 0 and (sts[7]["log_end_offset"], sts[7]["log_end_pos"]) == (1, 16)
    rows = e.scrub()
    assert e.last_scrub_rc == A.RMQ_OK
    U.assert_clean(rows, e, cfg)
    for p in range(cfg.num_partitions):  # the host walk agrees, replica by replica
        for r in range(3):
            assert U.host_walk(e, cfg, r, p)[1] == U.NONE
    part = e.scrub(2, 3)  # a sub-range names the same partitions
    assert np.array_equal(part, rows[2:5])


def test_clean_with_tickets_in_flight():
    # the scrub's own drain: batches submitted and never polled are applied before it looks
    cfg = U.cfg1()
    with Engine(cfg) as e:
        for b in range(3):
            e.append_async(*U.batch1(b))
        rows = e.scrub()
        assert e.last_scrub_rc == A.RMQ_OK
        assert e.state(0)["log_end_offset"] == 3 * len(U.LENS1)
        U.assert_clean(rows, e, cfg)


def test_clean_large_records(state2):
    e, cfg = state2
    rows = e.scrub()
    assert e.last_scrub_rc == A.RMQ_OK
    U.assert_clean(rows, e, cfg)
    S = cfg.segment_bytes
    recs = [x for p in range(4) for x in U.host_walk(e, cfg, 0, p)[2]]
    assert any(ln > 1024 and (pos % S) + 16 + ((ln + 15) & ~15) > S for _, pos, ln in recs), "a large record wraps"
    assert {ln for _, _, ln in recs} == set(U.LENS2)


def _pick(recs, S, what):
    """(record, byte delta from its start, mask) of a flip class in a clean record map."""
    def first(pred):  # (an inner record where there is one: the ends have their own cases)
        return next((x for x in recs[1:-1] if pred(x)), None) or next(x for x in recs if pred(x))
    if what == "payload":
        return first(lambda x: x[2] == 100), 16 + 50, 0x5A
    if what == "padding":
        return first(lambda x: x[2] == 17), 16 + 17 + 3, 0x5A
    if what == "crc":
        return first(lambda x: x[2] == 16), 12, 0x5A
    if what == "offset":
        return first(lambda x: x[2] == 600), 0, 0x5A
    if what == "len_low":  # 241 -> 240: one piece shorter, the record still fits its segment
        return first(lambda x: x[2] == 241), 8, 0x01
    if what == "len_top":  # the claimed length exceeds the ring
        return first(lambda x: x[2] == 15), 11, 0x5A
    if what == "straddle":  # a payload byte stored past the ring end
        x = next(x for x in recs if (x[1] % S) + 16 + x[2] > S)
        return x, S - (x[1] % S) + 8, 0x5A
    if what == "big_tail":  # past the first kilobyte of the 5000-byte record
        return next(x for x in recs if x[2] == 5000), 16 + 3000, 0x5A
    if what == "first":
        return recs[0], (16 if recs[0][2] else 12), 0x5A
    if what == "last":
        return recs[-1], (16 if recs[-1][2] else 12), 0x5A
    raise ValueError(what)


KINDS = {"payload": {CRC}, "padding": {CRC}, "crc": {CRC}, "offset": {CHAIN}, "len_low": {CRC, CHAIN},
         "len_top": {CHAIN}, "straddle": {CRC}, "big_tail": {CRC}, "first": {CRC}, "last": {CRC}}


def _flip_case(e, cfg, p, what, slot=2):
    S = cfg.segment_bytes
    clean = U.clean_totals(e, cfg)
    recs = U.host_walk(e, cfg, slot, p)[2]
    rec, delta, mask = _pick(recs, S, what)
    ring_off = (rec[1] + delta) % S
    e.fault_flip_ring(slot, p, ring_off, mask)
    try:
        rows = e.scrub()
        rc = e.last_scrub_rc
        k, bad, _, _ = U.host_walk(e, cfg, slot, p)
    finally:
        e.fault_flip_ring(slot, p, ring_off, mask)  # back
    assert bad == rec[0] and k == rec[0] - recs[0][0], (what, bad, rec)  # the host walk stops at the flipped record
    r = rows[p]
    print(what, "row", r, "host", bad)
    assert rc == A.RMQ_ECORRUPT and int(r["status"]) == A.RMQ_ECORRUPT
    assert (int(r["bad_offset"]), int(r["bad_replica"])) == (bad, slot), (what, r, bad)
    assert int(r["bad_kind"]) in KINDS[what], (what, r)
    assert int(r["replicas"]) == 3 and int(r["records_ok"]) <= 3 * clean[p][0] - 1, (what, r)
    for q in range(cfg.num_partitions):  # the other partitions' rows stay clean
        if q != p:
            n, nb = clean[q]
            assert (int(rows[q]["status"]), int(rows[q]["bad_offset"]), int(rows[q]["records_ok"]),
                    int(rows[q]["bytes_ok"])) == (A.RMQ_OK, U.NONE, 3 * n, 3 * nb), (what, q, rows[q])
    rows = e.scrub()  # flipped back: clean again
    assert e.last_scrub_rc == A.RMQ_OK
    U.assert_clean(rows, e, cfg)


@pytest.mark.parametrize("what", ["payload", "padding", "crc", "offset", "len_low", "len_top", "straddle",
                                  "first", "last"])
def test_flip_classes(state1, what):
    e, cfg = state1
    _flip_case(e, cfg, 0 if what == "straddle" else 3, what)


def test_flip_large_record_tail(state2):
    e, cfg = state2
    p = next(p for p in range(4) if any(x[2] == 5000 for x in U.host_walk(e, cfg, 2, p)[2]))
    _flip_case(e, cfg, p, "big_tail")


def test_lowest_offset_then_lowest_slot(state1):
    e, cfg = state1
    S, p = cfg.segment_bytes, 4
    recs = U.host_walk(e, cfg, 0, p)[2]
    lo, hi = recs[3], recs[9]
    a0, a2 = (hi[1] + 12) % S, (lo[1] + 12) % S  # a crc byte each: slot 0 at the higher offset, slot 2 at the lower
    e.fault_flip_ring(0, p, a0)
    e.fault_flip_ring(2, p, a2)
    try:
        r = e.scrub()[p]
        assert (U.host_walk(e, cfg, 0, p)[1], U.host_walk(e, cfg, 2, p)[1]) == (hi[0], lo[0])
    finally:
        e.fault_flip_ring(0, p, a0)
        e.fault_flip_ring(2, p, a2)
    assert (int(r["bad_offset"]), int(r["bad_replica"]), int(r["bad_kind"])) == (lo[0], 2, CRC), r
    e.fault_flip_ring(0, p, a2)  # the same offset on slots 0 and 2: the lower slot is named
    e.fault_flip_ring(2, p, a2)
    try:
        r = e.scrub()[p]
    finally:
        e.fault_flip_ring(0, p, a2)
        e.fault_flip_ring(2, p, a2)
    assert (int(r["bad_offset"]), int(r["bad_replica"]), int(r["bad_kind"])) == (lo[0], 0, CRC), r
    U.assert_clean(e.scrub(), e, cfg)


def test_range_and_argument_errors(state1):
    e, cfg = state1
    P = cfg.num_partitions
    for first, n in ((0, P + 1), (P, 1), (P + 1, 0), (3, P - 2)):
        with pytest.raises(EngineError) as ei:
            e.scrub(first, n)
        assert ei.value.status == A.RMQ_ENOPART, (first, n)
    assert len(e.scrub(P, 0)) == 0 and len(e.scrub(0, 0)) == 0  # an empty range inside [0, P]
    for args in ((0, 0, cfg.segment_bytes, 0x5A), (0, 0, 1 << 40, 0x5A), (0, 0, 16, 0), (0, 0, 16, 0x100), (3, 0, 16, 1)):
        with pytest.raises(EngineError) as ei:
            e.fault_flip_ring(*args)
        assert ei.value.status == A.RMQ_EINVAL, args
    U.assert_clean(e.scrub(), e, cfg)  # nothing was flipped


def test_profile_regions_of_scrub_repair_reindex():
    """rmq_profile_query's regions 2 (scrub), 5 (repair) and 8 (reindex): one pair of events per call,
    from before its first kernel to after its last; a scrub inside another call adds none to 2."""
    cfg = U.cfg1()
    with Engine(cfg) as e:
        U.fill1(e, 1)
        e.profile(1)
        e.scrub(), e.repair(), e.reindex()
        assert (e.last_scrub_rc, e.last_repair_rc, e.last_reindex_rc) == (A.RMQ_OK,) * 3
        first = {k: e.profile_query(k) for k in (2, 5, 8)}
        print("one call each:", first)
        for k, (calls, ms) in first.items():
            assert calls == 1 and ms > 0, (k, calls, ms)
        assert e.profile_query(6)[0] == 0 and e.profile_query(7)[0] == 0
        S, p = cfg.segment_bytes, 0
        rec = next(x for x in U.host_walk(e, cfg, 2, p)[2] if x[2] == 100)
        e.fault_flip_ring(2, p, (rec[1] + 16 + 50) % S)  # a payload byte: the repair copies and scrubs again
        row = e.repair()[p]
        assert e.last_repair_rc == A.RMQ_OK and int(row["segments_repaired"]) == 1, row
        calls, ms = e.profile_query(5)
        print("second repair:", calls, ms)
        assert calls == 2 and ms > first[5][1], (calls, ms, first[5])
        assert e.profile_query(2)[0] == 1  # the repair's scrub is inside region 5
        U.assert_clean(e.scrub(), e, cfg)


def test_after_ring_move():
    cfg = U.cfg1(pool_bytes=16 * 4096)
    with Engine(cfg) as e:
        U.fill1(e)
        before = e.state(1)
        e.set_segments([1, 2], [2048, 16384])  # one shrinks (retention at the new size first), one grows
        e.append(*U.batch1(U.BATCHES1))        # and the moved rings keep taking records
        st1, st2 = e.state(1), e.state(2)
        assert (st1["segment_bytes"], st2["segment_bytes"]) == (2048, 16384)
        assert st1["log_start_offset"] > before["log_start_offset"]
        rows = e.scrub()
        assert e.last_scrub_rc == A.RMQ_OK
        U.assert_clean(rows, e, cfg)
        for p in (1, 2):  # a flip in the moved ring is found where the host walk finds it
            S = e.state(p)["segment_bytes"]
            recs = U.host_walk(e, cfg, 1, p)[2]
            rec = recs[len(recs) // 2]
            off = (rec[1] + 12) % S
            e.fault_flip_ring(1, p, off)
            r = e.scrub()[p]
            bad = U.host_walk(e, cfg, 1, p)[1]
            e.fault_flip_ring(1, p, off)
            assert bad == rec[0]
            assert (int(r["status"]), int(r["bad_offset"]), int(r["bad_replica"]), int(r["bad_kind"])) == \
                (A.RMQ_ECORRUPT, bad, 1, CRC), (p, r)
        U.assert_clean(e.scrub(), e, cfg)


def _run_ranks(world, body, timeout=120):
    errs = [None] * world

    def wrap(r):
        try:
            body(r)
        except BaseException as ex:  # noqa: BLE001 - reported below
            errs[r] = ex

    ts = [threading.Thread(target=wrap, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
        assert not t.is_alive(), "a rank hung"
    for r, ex in enumerate(errs):
        if ex is not None:
            raise AssertionError(f"rank {r}: {ex!r}") from ex


def _assert_rank_clean(e, cfg, view, rank, rows):
    for p in range(cfg.num_partitions):
        slots = [s for s in range(cfg.replication_factor) if view.ranks[p][s] == rank]
        st = e.state(p)
        n, nb = st["log_end_offset"] - st["log_start_offset"], st["log_end_pos"] - st["log_start_pos"]
        r = rows[p]
        for s in slots:
            assert U.host_walk(e, cfg, s, p)[1] == U.NONE, (rank, p, s)  # the host walk accepts the bytes
        assert (int(r["status"]), int(r["bad_offset"]), int(r["replicas"]), int(r["records_ok"]), int(r["bytes_ok"])) == \
            (A.RMQ_OK, U.NONE, len(slots), len(slots) * n, len(slots) * nb), (rank, p, r, st)


def test_after_follower_truncation():
    # tests/repl_sim.py's leader-change script (as test_gpu_replication.py runs it): rank 0's third
    # round is lost and the leadership of its partitions moves, so rank 0 cuts its divergent tail
    # and follows at term 2. Every engine then scrubs clean, led and followed partitions alike.
    world, rf, ppr, group = 3, 3, 6, 2
    spec = StreamSpec(ppr, 300, "uniform", size=(0, 120), config_index=71)
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=1 << 16, index_interval=256,
                        max_batch_records=4096, max_batch_bytes=1 << 20, pipeline_depth=group)
    views, new, phases = leader_change_script(spec, world, rf, ppr, group)
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    hub = LocalHub(world)
    engs = [Engine(c) for c in cfgs]
    rows = [None] * world
    final = [views[r] for r in range(world)]
    try:
        def body(r):
            e = engs[r]
            e.attach_local(hub)
            place(e, views[r])
            for k, (batches, drop, placement, bl) in enumerate(phases):
                if placement is not None:
                    place(e, placement[r])
                    final[r] = placement[r]
                    for p, t in bl[r]:
                        e.become_leader(p, t)
                if r in drop:
                    e.fault_drop_rounds(1)
                for b in batches[r]:
                    e.append_async(b.pidx, b.lens, b.payload)
                if k != 2:
                    e.sync()
            e.sync()
            rows[r] = e.scrub()  # collective, like the sync before it
            assert e.last_scrub_rc == A.RMQ_OK

        _run_ranks(world, body)
        stats = [e.replication_stats() for e in engs]
        assert all(s["refused_log"] > 0 for s in stats[1:]), stats  # the lost round was missed
        for p in range(ppr):  # rank 0 truncated and follows its former partitions at term 2
            st = engs[0].state(p)
            assert st["term"] == 2 and not st["is_leader"] and st["log_end_offset"] > 0
        for r in range(world):
            assert sum(int(x) for x in rows[r]["records_ok"]) > 0
            _assert_rank_clean(engs[r], cfgs[r], final[r], r, rows[r])
    finally:
        for e in engs:
            e.close()
        hub.close()


def test_after_follower_rebase():
    # rank 0's regions are lost for 9 rounds (as test_follower_beyond_the_ring_rebases_gpu): its
    # followers fall more than the 8 KB ring behind and are rebased at the leader's rebase point
    world, rf, rounds = 3, 3, 12
    spec = StreamSpec(1, 10, "uniform", size=(100, 100), config_index=58)
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=1 << 13, index_interval=256,
                        max_batch_records=4096, max_batch_bytes=1 << 20, pipeline_depth=1)
    views = [rank_view(r, world, 1, rf) for r in range(world)]
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    hub = LocalHub(world)
    engs = [Engine(c) for c in cfgs]
    rows = [None] * world
    try:
        def body(r):
            e = engs[r]
            e.attach_local(hub)
            place(e, views[r])
            for k in range(rounds):
                if r == 0 and k < 9:
                    e.fault_drop_rounds(1)
                b = make_batch(spec, 1000 * r + 50 * k)
                e.append_async(b.pidx, b.lens, b.payload)
                e.sync()
            rows[r] = e.scrub()
            assert e.last_scrub_rc == A.RMQ_OK

        _run_ranks(world, body)
        lead = engs[0].state(0)
        assert lead["log_start_offset"] > 0 and min(lead["match"][:rf]) == lead["log_end_offset"], lead
        for r in (1, 2):  # the followers' copies of rank 0's partition restarted past their old ends
            p = next(p for p in range(cfgs[r].num_partitions) if views[r].ranks[p][0] == 0)
            st = engs[r].state(p)
            assert st["log_start_offset"] > 0 and st["log_end_offset"] == lead["log_end_offset"], (r, st)
        for r in range(world):
            _assert_rank_clean(engs[r], cfgs[r], views[r], r, rows[r])
    finally:
        for e in engs:
            e.close()
        hub.close()
