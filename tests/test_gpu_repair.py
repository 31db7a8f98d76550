"""rmq_repair on the GPU (FORMAT.md §10, "Repair"): clean logs, one flip per class, several pairs in
one call, bytes outside the log, the every-byte sweep, the length edges, many partitions and the
grid cap, moved rings, followers over a transport, arguments and the read processor. Every expected
ring and counter comes from the host model (tests/repair_util.py, checked on the CPU by
tests/test_repair_model.py) over bytes read back before the damage, never from rmq_repair."""
import time

import numpy as np
import pytest

import repair_util as R
import scrub_util as U
from repl_sim import place, rank_cfg
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine, EngineConfig, EngineError, LocalHub, parse_records
from ripplemq_amd.sharding import rank_view
from ripplemq_amd.state_machine import MessageBatchReadRequest, PartitionBroker, PartitionDirectory
from ripplemq_amd.workload import StreamSpec, make_batch
from test_gpu_scrub import _run_ranks

pytestmark = pytest.mark.gpu

OK, ECORRUPT = A.RMQ_OK, A.RMQ_ECORRUPT
ROW = ["bad_offset", "bad_replica", "bad_kind", "replicas", "status"]


def _engine(cfg, fill):
    e = Engine(cfg)
    fill(e)
    return e


@pytest.fixture()
def fresh1():
    e = _engine(U.cfg1(), U.fill1)
    yield e, U.cfg1()
    e.close()


@pytest.fixture(scope="module")
def state1():
    e = _engine(U.cfg1(), U.fill1)
    yield e, U.cfg1()
    e.close()


@pytest.fixture(scope="module")
def state2():
    e = _engine(U.cfg2(), U.fill2)
    yield e, U.cfg2()
    e.close()


def _counts(rows, first=0):
    return {first + i: (int(r["segments_repaired"]), int(r["bytes_repaired"]), int(r["segments_unrepaired"]))
            for i, r in enumerate(rows)}


def _assert_rings(e, want, what=""):
    for p, rs in want.items():
        n = rs[next(iter(rs))].size
        for r, a in rs.items():
            got = e.read_segment(r, p, 0, n)
            assert np.array_equal(got, a), (what, p, r, np.flatnonzero(got != a)[:8])


def _same_rows(rep, scrub):
    return all(np.array_equal(rep[f], scrub[f]) for f in ROW)


def _damage_and_repair(e, cfg, flips, parts=None, first=0, n=None, dry=True, slots=None):
    """Snapshot, model, flip, (dry run,) repair, scrub: the checks every scenario shares. Returns
    (repair rows, return value, the following scrub's rows, the clean snapshot)."""
    snap = R.snapshot(e, cfg, parts, slots)
    bad = R.apply_flips(snap, flips)
    want_rings, want_counts = R.model(bad, cfg.index_interval)
    for f in flips:
        e.fault_flip_ring(*f)
    if dry:
        before = e.scrub(first, n)
        d = e.repair(first, n, dry_run=True)
        assert e.last_repair_rc == e.last_scrub_rc
        got = _counts(d, first)
        assert {p: got[p] for p in want_counts} == want_counts, (got, want_counts)
        assert _same_rows(d, before)  # the present state: the scrub's row
        _assert_rings(e, {p: rs for p, (_, _, rs) in bad.items()}, "dry run")  # nothing written
    rows = e.repair(first, n)
    rc = e.last_repair_rc
    after = e.scrub(first, n)
    assert rc == e.last_scrub_rc and _same_rows(rows, after), (rows, after)
    got = _counts(rows, first)
    assert {p: got[p] for p in want_counts} == want_counts, (got, want_counts)
    assert all(c == (0, 0, 0) for p, c in got.items() if p not in want_counts)
    _assert_rings(e, want_rings, "repair")
    return rows, rc, after, snap


def _clean_rings(snap):
    return {p: rs for p, (_, _, rs) in snap.items()}


# ---- clean logs
@pytest.mark.parametrize("which", [1, 2])
def test_clean_logs(state1, state2, which):
    e, cfg = state1 if which == 1 else state2
    snap = R.snapshot(e, cfg)
    scrub = e.scrub()
    for dry in (True, False):
        rows = e.repair(dry_run=dry)
        assert e.last_repair_rc == OK and _same_rows(rows, scrub)
        assert all(c == (0, 0, 0) for c in _counts(rows).values())
    _assert_rings(e, _clean_rings(snap))
    U.assert_clean(e.scrub(), e, cfg)
    assert _same_rows(e.repair(2, 3), rows[2:5])  # a sub-range names the same partitions


# ---- one flip per class
def _class_case(e, cfg, what, p):
    S = cfg.segment_bytes
    recs = U.host_walk(e, cfg, R.CLASS_SLOT, p)[2]
    rec, flip = R.class_flip(recs, S, what, p)
    st = e.state(p)
    segs = R.segments(st, R.snapshot(e, cfg, [p])[p][1], cfg.index_interval)
    seg = segs[R.seg_of(segs, rec[1])]
    rows, rc, after, snap = _damage_and_repair(e, cfg, [flip])
    assert rc == OK and _counts(rows)[p] == (1, seg[1] - seg[0], 0), (what, rows[p])
    _assert_rings(e, _clean_rings(snap), what)  # slot 2 healed, slots 0 and 1 untouched, every other ring too
    U.assert_clean(after, e, cfg)  # records_ok = 3 n
    # a verified fetch of the slice is served
    e.commit_consumer_offset(np.array([p], np.uint32), np.array([0], np.uint32), np.array([rec[0]], np.uint64))
    rc, res, buf, _ = e.fetch(np.array([p]), np.array([0]), np.array([1]), verify=True)
    assert rc == OK and int(res["status"][0]) == OK and int(res["count"][0]) == 1
    got = parse_records(buf[int(res["out_pos"][0]):int(res["out_pos"][0]) + int(res["bytes"][0])])
    assert [(o, len(b)) for o, _, b in got] == [(rec[0], rec[2])]
    return seg


@pytest.mark.parametrize("what", R.CLASSES1)
def test_flip_classes(state1, what):
    e, cfg = state1
    seg = _class_case(e, cfg, what, R.class_partition(what))
    if what == "straddle":
        assert seg[0] % cfg.segment_bytes > (seg[1] - 1) % cfg.segment_bytes  # the segment wraps the ring end


def test_flip_large_record_tail(state2):
    e, cfg = state2
    p = next(p for p in range(4) if any(x[2] == 5000 for x in U.host_walk(e, cfg, 2, p)[2]))
    seg = _class_case(e, cfg, "big_tail", p)
    assert seg[1] - seg[0] > 1024  # several 1 KiB steps of the wave's copy


# ---- several pairs in one call
@pytest.mark.parametrize("which", ["distinct", "same", "all3"])
def test_several_pairs(fresh1, which):
    e, cfg = fresh1
    p = R.MULTI_P
    recs4, recs5 = U.host_walk(e, cfg, 0, p)[2], U.host_walk(e, cfg, 0, R.OTHER_P)[2]
    segs = R.segments(e.state(p), R.snapshot(e, cfg, [p])[p][1], cfg.index_interval)
    flips = R.multi_flips(recs4, recs5, segs, cfg.segment_bytes, which)
    rows, rc, after, snap = _damage_and_repair(e, cfg, flips)
    c = _counts(rows)
    assert c[R.OTHER_P][0] == 1 and int(rows[R.OTHER_P]["status"]) == OK  # the second partition is repaired
    if which == "all3":
        assert rc == ECORRUPT and c[p] == (0, 0, 3) and int(rows[p]["status"]) == ECORRUPT
        want = min(U.host_walk(e, cfg, r, p)[1] for r in range(3))  # the host walk's offset
        assert int(rows[p]["bad_offset"]) == int(after[p]["bad_offset"]) == want
        bad = R.apply_flips(snap, flips)
        _assert_rings(e, {p: bad[p][2]}, "all3")  # every byte unchanged
    else:
        assert rc == OK and c[p][0] == 2 and c[p][2] == 0
        _assert_rings(e, _clean_rings(snap), which)
        U.assert_clean(after, e, cfg)


def test_byte_outside_the_log_is_not_repaired(fresh1):
    e, cfg = fresh1
    st = e.state(7)
    assert (st["log_end_offset"], st["log_end_pos"]) == (1, 16)
    clean = e.read_segment(2, 7, 0, cfg.segment_bytes)
    flips = [(2, 7, 16, 0x5A), (2, 7, 1000, 0x5A)]
    rows, rc, after, _ = _damage_and_repair(e, cfg, flips)
    assert rc == OK and _counts(rows)[7] == (0, 0, 0)
    got = e.read_segment(2, 7, 0, cfg.segment_bytes)
    assert list(np.flatnonzero(got != clean)) == [16, 1000]  # neither reported nor rewritten: still flipped


# ---- the every-byte sweep
def test_every_byte_sweep(fresh1):
    """Every byte of partition 3's retained log flipped on slot 2, one repair each (3,376 calls, no
    stride: scrub_util.SWEEP_STRIDE stays None). The sweep's time is printed."""
    e, cfg = fresh1
    S, p, slot = cfg.segment_bytes, U.SWEEP_P, U.SWEEP_SCRUB_SLOT
    st = e.state(p)
    clean = e.read_segment(slot, p, 0, S)
    win = clean[np.arange(st["log_start_pos"], st["log_end_pos"]) % S]
    recs = U.walk_window(win, st)[2]
    flips = U.sweep_positions(recs)
    assert [w for w, _, _ in flips] == list(range(win.size))
    wrong = []
    t0 = time.perf_counter()
    for w, i, d in flips:
        e.fault_flip_ring(slot, p, (st["log_start_pos"] + w) % S, U.SWEEP_MASK)
        rows = e.repair()
        if not (e.last_repair_rc == OK and int(rows[p]["segments_repaired"]) == 1 and
                int(rows["segments_repaired"].sum()) == 1 and not rows["segments_unrepaired"].any() and
                np.array_equal(e.read_segment(slot, p, 0, S), clean)):
            wrong.append((w, i, d, rows[p]))
            break  # (the ring is no longer the clean one)
    print(f"repair sweep: {len(flips)} flips in {time.perf_counter() - t0:.2f} s")
    assert not wrong, wrong
    U.assert_clean(e.scrub(), e, cfg)


# ---- state 3: RF 2, the length edges
def test_length_edges():
    cfg = U.cfg3()
    with Engine(cfg) as e:
        U.fill3(e)
        S, p = cfg.segment_bytes, 1
        recs = U.host_walk(e, cfg, 1, p)[2]
        picks = [next(x for x in recs if x[2] == ln) for ln in U.BIG3]
        picks += [next(x for x in recs if x[2] == ln) for ln in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48)]
        flips = [(1, p, (x[1] + (16 + x[2] // 2 if x[2] else 12)) % S, 0x5A) for x in picks]
        rows, rc, after, snap = _damage_and_repair(e, cfg, flips, parts=[p])
        assert rc == OK and _counts(rows)[p][0] > 20 and _counts(rows)[p][2] == 0
        _assert_rings(e, _clean_rings(snap))
        U.assert_clean(after, e, cfg)


# ---- state 4: 2,500 partitions, sub-ranges, the grid cap
def _marked_flips(e, cfg):
    out = []
    for k, p in enumerate(U.MARKED4):
        recs = U.host_walk(e, cfg, k % 2, p)[2]
        out.append((k % 2, p, (recs[len(recs) // 2][1] + 12) % cfg.segment_bytes, 0x5A))
    return out


@pytest.mark.parametrize("wgs", [None, "1"])
def test_many_partitions(monkeypatch, wgs):
    if wgs:
        monkeypatch.setenv("RMQ_AUDIT_WGS", wgs)  # (read at rmq_create) one workgroup: the stride loops run
    cfg = U.cfg4()
    with Engine(cfg) as e:
        U.fill4(e)
        states = e.states()
        flips = _marked_flips(e, cfg)
        near = [p for m in U.MARKED4 for p in (m - 1, m, m + 1) if 0 <= p < U.P4]
        # a sub-range that starts inside a plan chunk: 1023, 1024, 2047 and 2048 lie in it
        sub = [f for f in flips if 1000 <= f[1] < 2100]
        rows, rc, after, snap = _damage_and_repair(e, cfg, sub, parts=[p for p in near if 1000 <= p < 2100], first=1000,
                                                   n=1100)
        assert rc == OK and int(rows["segments_repaired"].sum()) == 4 and not rows["segments_unrepaired"].any()
        U.assert_clean_bulk(after, states[1000:2100], 2)
        rows, rc, after, snap = _damage_and_repair(e, cfg, flips, parts=near)
        assert rc == OK and int(rows["segments_repaired"].sum()) == 8 and not rows["segments_unrepaired"].any()
        assert sorted(np.flatnonzero(rows["segments_repaired"])) == sorted(U.MARKED4)
        _assert_rings(e, _clean_rings(snap))
        U.assert_clean_bulk(after, states, 2)


# ---- after set_segments
def test_after_ring_move():
    cfg = U.cfg1(pool_bytes=16 * 4096)
    with Engine(cfg) as e:
        U.fill1(e)
        e.set_segments([1, 2], [2048, 16384])  # one shrinks, one grows
        e.append(*U.batch1(U.BATCHES1))
        assert (e.state(1)["segment_bytes"], e.state(2)["segment_bytes"]) == (2048, 16384)
        flips = []
        for p in (1, 2):
            recs = U.host_walk(e, cfg, 1, p)[2]
            flips.append((1, p, (recs[len(recs) // 2][1] + 12) % e.state(p)["segment_bytes"], 0x5A))
        rows, rc, after, snap = _damage_and_repair(e, cfg, flips)
        assert rc == OK and [_counts(rows)[p][0] for p in (1, 2)] == [1, 1]
        _assert_rings(e, _clean_rings(snap))
        U.assert_clean(after, e, cfg)


# ---- with a transport
def _world(world, rf, body_after):
    spec = StreamSpec(2, 40, "uniform", size=(0, 200), config_index=71)
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=1 << 14, index_interval=256,
                        max_batch_records=4096, max_batch_bytes=1 << 20, pipeline_depth=1)
    views = [rank_view(r, world, 2, rf) for r in range(world)]
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    hub = LocalHub(world)
    engs = [Engine(c) for c in cfgs]
    try:
        def body(r):
            e = engs[r]
            e.attach_local(hub)
            place(e, views[r])
            for k in range(4):  # a handful of batches, no dropped rounds
                b = make_batch(spec, 1000 * r + k)
                e.append_async(b.pidx, b.lens, b.payload)
                e.sync()
            e.sync()
            body_after(r, e, cfgs[r], views[r])

        _run_ranks(world, body)
    finally:
        for e in engs:
            e.close()
        hub.close()


def _local_slots(view, rank, rf):
    return lambda p: [s for s in range(rf) if view.ranks[p][s] == rank]


def test_follower_with_two_slots_is_repaired():
    # world 2, RF 3: both followers of a partition sit on the other rank, two slots there
    def after(r, e, cfg, view):
        slots = _local_slots(view, r, 3)
        flips = []
        if r == 1:
            p = next(p for p in range(cfg.num_partitions) if slots(p) == [1, 2] and e.state(p)["log_end_offset"] > 3)
            recs = U.host_walk(e, cfg, 2, p)[2]
            flips = [(2, p, (recs[len(recs) // 2][1] + 12) % cfg.segment_bytes, 0x5A)]
        rows, rc, scrub, snap = _damage_and_repair(e, cfg, flips, slots=slots, dry=False)  # collective
        assert rc == OK and int(rows["segments_repaired"].sum()) == len(flips)
        if flips:
            assert _counts(rows)[flips[0][1]][0] == 1
        _assert_rings(e, _clean_rings(snap))
        assert e.last_scrub_rc == OK and (scrub["status"] == OK).all()  # every rank's scrub is clean

    _world(2, 3, after)


def test_follower_with_one_slot_is_not():
    # world 3, RF 3: every rank holds one slot of a partition, so a follower has no donor
    def after(r, e, cfg, view):
        slots = _local_slots(view, r, 3)
        flips = []
        if r == 1:
            p = next(p for p in range(cfg.num_partitions) if slots(p) and slots(p)[0] != 0 and e.state(p)["log_end_offset"] > 3)
            recs = U.host_walk(e, cfg, slots(p)[0], p)[2]
            flips = [(slots(p)[0], p, (recs[len(recs) // 2][1] + 12) % cfg.segment_bytes, 0x5A)]
        rows, rc, scrub, snap = _damage_and_repair(e, cfg, flips, slots=slots, dry=False)
        if r == 1:
            p = flips[0][1]
            assert rc == ECORRUPT and _counts(rows)[p] == (0, 0, 1) and int(rows["segments_unrepaired"].sum()) == 1
            _assert_rings(e, {p: R.apply_flips(snap, flips)[p][2]})  # bytes unchanged
        else:
            assert rc == OK and not rows["segments_unrepaired"].any()

    _world(3, 3, after)


# ---- arguments
def test_range_and_argument_errors(state1):
    e, cfg = state1
    P = cfg.num_partitions
    for first, n in ((0, P + 1), (P, 1), (P + 1, 0), (3, P - 2)):
        with pytest.raises(EngineError) as ei:
            e.repair(first, n)
        assert ei.value.status == A.RMQ_ENOPART, (first, n)
    assert len(e.repair(P, 0)) == 0 and len(e.repair(0, 0)) == 0 and e.last_repair_rc == OK
    for flags in (2, 3, 0x80000000):  # an unknown flag bit
        assert e.lib.rmq_repair(e.h, 0, 1, flags, None) == A.RMQ_EINVAL
    assert e.lib.rmq_repair(e.h, 0, P, 0, None) == OK  # res is nullable
    U.assert_clean(e.scrub(), e, cfg)


# ---- the read processor
@pytest.mark.parametrize("case", ["healed", "all3", "off"])
def test_read_processor(fresh1, case):
    e, cfg = fresh1
    S, p = cfg.segment_bytes, 3
    st = e.state(p)
    lo = st["log_start_offset"]
    e.commit_consumer_offset(np.array([p, 1], np.uint32), np.zeros(2, np.uint32),
                             np.array([lo, e.state(1)["log_start_offset"]], np.uint64))
    d = PartitionDirectory({"t": cfg.num_partitions}, max_consumers=cfg.max_consumers)
    reqs = [MessageBatchReadRequest("c0", 8, "t", p), MessageBatchReadRequest("c0", 5, "t", 1)]
    want = PartitionBroker(d, engine=e, messages_as_str=False, verify=True).process_batch_read(reqs)
    assert all(x.isSuccess() for x in want) and len(want[0].getMessages()) == 8
    clean = {r: e.read_segment(r, p, 0, S) for r in range(3)}
    rec = next(x for x in U.host_walk(e, cfg, 0, p)[2][:8] if x[2] > 0)
    for slot in ((0, 1, 2) if case == "all3" else (0,)):
        e.fault_flip_ring(slot, p, (rec[1] + 16) % S)
    br = PartitionBroker(d, engine=e, messages_as_str=False, verify=True, repair=case != "off")
    out = br.process_batch_read(reqs)
    today = PartitionBroker(d, engine=e, messages_as_str=False, verify=True).process_batch_read(reqs) if case != "healed" else None
    assert out[1].isSuccess() and out[1].getMessages() == want[1].getMessages()
    if case == "healed":
        assert out[0].isSuccess() and out[0].getMessages() == want[0].getMessages() and out[0].getOffset() == want[0].getOffset()
        for r in range(3):
            assert np.array_equal(e.read_segment(r, p, 0, S), clean[r])  # the ring is healed
        U.assert_clean(e.scrub(), e, cfg)
    else:  # exactly today's failed response
        for x in (out[0], today[0]):
            assert not x.isSuccess() and x.getMessages() == [] and "t-3" in x.getErrorMsg() and x.getOffset() == lo
        assert out[0].getErrorMsg() == today[0].getErrorMsg()
        assert not np.array_equal(e.read_segment(0, p, 0, S), clean[0])
