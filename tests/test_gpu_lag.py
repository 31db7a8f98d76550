"""rmq_lag on the GPU (FORMAT.md §7 "Lag"): every expected value is lag_util.model_lag on an oracle run
of the same scenario (tests/test_lag_model.py shows that the model agrees with the oracle's fetch,
that its headroom is the edge it claims and that the request lists here hold their categories)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import lag_util as L
import scrub_util as U
from repl_sim import exchange_round, notice_round, place, rank_batches, rank_cfg
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import LAG_RES_DTYPE, Engine, EngineConfig, EngineError, LocalHub
from ripplemq_amd.sharding import rank_view
from ripplemq_amd.state_machine import PartitionBroker, PartitionDirectory
from ripplemq_amd.tier import DurableLog
from ripplemq_amd.workload import StreamSpec
from test_gpu_replication import run_ranks

pytestmark = pytest.mark.gpu

NONE = L.NONE


def lag_device_rows(e, pidx, cons, offs=None, flags=0) -> np.ndarray:
    """The same call with rows, offsets and result rows in device memory."""
    n = len(pidx)
    d_req, d_res, d_at = e.device_alloc(16 * n), e.device_alloc(64 * n), e.device_alloc(8 * n)
    try:
        e.h2d(d_req, L.reqs_array(pidx, cons, flags).view(np.uint8).reshape(-1))
        e.h2d(d_res, np.full(64 * n, 0xEE, np.uint8))
        if offs is not None:
            e.h2d(d_at, np.ascontiguousarray(offs, np.uint64).view(np.uint8))
        e.lag_device(d_req, d_at if offs is not None else None, n, d_res)
        rows = np.zeros(n, LAG_RES_DTYPE)
        e.d2h(rows.view(np.uint8), d_res)
        return rows
    finally:
        for d in (d_req, d_res, d_at):
            e.device_free(d)


# ---- 1: the sweep on state 1
def test_sweep_on_state_1(oracle_mod):
    e, cfg = L.filled1(Engine)
    ora, _ = L.filled1(oracle_mod.OracleEngine)
    with e, ora:
        pidx, cons, offs = L.sweep_reqs1(ora)
        want = L.model_lag(ora, pidx, cons, offs)
        assert (want["status"] == A.RMQ_EOFFSET).any() and (want["records"] > 0).sum() > 60
        snap = L.snapshot(e)
        host = e.lag(pidx, cons, offsets=offs)
        L.assert_rows(host, want, "host rows")
        dev = lag_device_rows(e, pidx, cons, offs)
        L.assert_rows(dev, want, "device rows")
        assert host.tobytes() == dev.tobytes()
        L.assert_unchanged(e, snap)
        # the same offsets committed, no explicit offsets (null, and an array of RMQ_OFFSET_NONE)
        for pp, cc, oo in L.commit_rounds1(ora):
            for x in (e, ora):
                rc, st = x.commit_consumer_offset(pp, cc, oo)
                assert rc == 0 and not st.any()
            want = L.model_lag(ora, pp, cc)
            snap = L.snapshot(e)
            host = e.lag(pp, cc)
            L.assert_rows(host, want, ("committed", int(oo[0])))
            L.assert_rows(e.lag(pp, cc, offsets=np.full(len(pp), NONE, np.uint64)), want, "none")
            assert lag_device_rows(e, pp, cc).tobytes() == host.tobytes()
            L.assert_unchanged(e, snap)


# ---- 2: a high watermark inside the log (end_pos by a search) and below the log start
def test_high_watermark_inside_the_log(oracle_mod):
    cfg = U.cfg1()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        L.scenario2(e), L.scenario2(ora)
        for p in L.LAGGING2:
            assert e.state(p) == ora.state(p)
        st = ora.state(L.LAGGING2[0])
        lo, hw, leo = st["log_start_offset"], st["high_watermark"], st["log_end_offset"]
        assert lo < hw < leo
        pidx, cons, offs = L.reqs2(ora)
        want = L.model_lag(ora, pidx, cons, offs)
        served = want[(pidx == L.LAGGING2[0]) & (want["records"] > 0)]
        assert len(served) >= hw and (served["end_pos"] < st["log_end_pos"]).all()  # not the log end's position
        both = offs[(pidx == L.LAGGING2[0])]
        assert {hw - 1, hw, hw + 1, leo, leo + 1} <= set(both.tolist())
        L.assert_rows(e.lag(pidx, cons, offsets=offs), want, "host rows")
        L.assert_rows(lag_device_rows(e, pidx, cons, offs), want, "device rows")


# ---- 3: long records and a wide table
def test_long_records_and_a_wide_table(oracle_mod):
    cfg = U.cfg3()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        L.scenario3(e), L.scenario3(ora)
        pidx, cons = L.reqs3()
        want = L.model_lag(ora, pidx, cons)
        assert (want["status"] == A.RMQ_OK).all() and (want["bytes"] > 16384).any()
        L.assert_rows(e.lag(pidx, cons), want, "host rows")
        L.assert_rows(lag_device_rows(e, pidx, cons), want, "device rows")


# ---- 4: grid edges
def test_grid_edges_on_state_4(oracle_mod):
    cfg = U.cfg4()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        L.scenario4(e), L.scenario4(ora)
        pidx, cons, offs = L.reqs4()
        want = L.model_lag(ora, pidx, cons, offs)
        for s in (A.RMQ_ENOPART, A.RMQ_EINVAL, A.RMQ_ENOTLEADER, A.RMQ_OK):
            assert (want["status"] == s).any(), s
        for n in L.N4:
            L.assert_rows(e.lag(pidx[:n], cons[:n], offsets=offs[:n]), want[:n], n)
        L.assert_rows(lag_device_rows(e, pidx, cons, offs), want, "device rows")
        L.assert_rows(lag_device_rows(e, pidx[:L.WG + 1], cons[:L.WG + 1], offs[:L.WG + 1]), want[:L.WG + 1], "device rows, 17")


# ---- 5: offsets past 2^32, positions past 2^40
def test_past_2_32(oracle_mod):
    cfg = L.H.cfg_high()
    bases = L.high_bases(cfg.index_interval)
    assert bases[L.HIGH_P][0] > 2 ** 32 and bases[L.HIGH_P][1] > 2 ** 40 and bases[L.HIGH_P][1] % cfg.index_interval == 0
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        L.scenario5(e, bases, ora)
        pidx, cons, offs = L.reqs5(ora)
        want = L.shift_rows(L.model_lag(ora, pidx, cons, offs), pidx, bases)
        up = L.shift_offsets(offs, pidx, bases)
        st = e.state(L.HIGH_P)
        assert st["log_start_offset"] > 2 ** 32 + 5 and st["log_start_pos"] > 2 ** 40
        L.assert_rows(e.lag(pidx, cons, offsets=up), want, "host rows")
        L.assert_rows(lag_device_rows(e, pidx, cons, up), want, "device rows")


# ---- 6: replica rows
def test_replica_rows_without_a_transport(oracle_mod):
    cfg = U.cfg1()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        cur = L.scenario6(e)
        assert L.scenario6(ora) == cur
        assert e.state(L.FOLLOWED1) == ora.state(L.FOLLOWED1) and not e.state(L.FOLLOWED1)["is_leader"]
        p = np.array(list(cur), np.uint32)
        c = np.arange(len(p), dtype=np.uint32) % cfg.max_consumers
        plain = e.lag(p, c)
        L.assert_rows(plain, L.model_lag(ora, p, c), "plain")
        assert int(plain["status"][0]) == A.RMQ_ENOTLEADER and int(p[0]) == L.FOLLOWED1
        want = L.model_lag(ora, p, c, replica=True, cursor=cur)
        assert int(want["start_offset"][0]) == cur[L.FOLLOWED1] and int(want["records"][0]) > 0
        L.assert_rows(e.lag(p, c, replica=True), want, "replica")
        L.assert_rows(lag_device_rows(e, p, c, flags=A.RMQ_FETCH_REPLICA), want, "replica, device rows")
        # explicit offsets replace the cursor; the cursors stay
        offs = np.array([cur[int(x)] + 1 for x in p], np.uint64)
        L.assert_rows(e.lag(p, c, offsets=offs, replica=True), L.model_lag(ora, p, c, offs, replica=True), "explicit")
        L.assert_rows(e.lag(p, c, replica=True), want, "replica again")


def test_replica_rows_with_the_local_transport(oracle_mod):
    world, rf, ppr, group, rounds = 2, 2, 1, 2, 3
    spec = StreamSpec(ppr, 300, "uniform", size=(0, 400), config_index=76)
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=1 << 16, index_interval=256,
                        max_batch_records=4096, max_batch_bytes=1 << 20, pipeline_depth=group)
    views = [rank_view(r, world, ppr, rf) for r in range(world)]
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    batches = [rank_batches(spec, r, rounds, group) for r in range(world)]
    hub = LocalHub(world)
    engs = [Engine(c) for c in cfgs]
    got = [None] * world
    CUR = 5
    try:
        def body(r):  # every rank makes the same calls
            e = engs[r]
            e.attach_local(hub)
            place(e, views[r])
            for b in batches[r]:
                e.append_async(b.pidx, b.lens, b.payload)
            e.sync()
            followed = np.arange(views[r].led, len(views[r].gp), dtype=np.uint32)
            # (the rings have wrapped: the cursor goes CUR records into what the replica retains)
            cur = np.array([e.state(int(p))["log_start_offset"] + CUR for p in followed], np.uint64)
            e.set_replica_cursor(followed, cur)
            every = np.arange(len(views[r].gp), dtype=np.uint32)
            got[r] = (followed, e.lag(followed, np.zeros(len(followed), np.uint32)),
                      e.lag(followed, np.zeros(len(followed), np.uint32), replica=True),
                      e.lag(every, np.zeros(len(every), np.uint32), offsets=np.zeros(len(every), np.uint64), replica=True))
            e.sync()

        run_ranks(world, body)
        oras = [oracle_mod.OracleEngine(c) for c in cfgs]
        try:
            for r in range(world):
                place(oras[r], views[r], world)
            for k in range(rounds):
                for r in range(world):
                    for b in batches[r][k * group:(k + 1) * group]:
                        oras[r].append(b.pidx, b.lens, b.payload)
                exchange_round(oras)
            notice_round(oras)
            for r in range(world):
                followed, plain, rep, every = got[r]
                assert len(followed) == 1
                z = np.zeros(len(followed), np.uint32)
                assert (plain["status"] == A.RMQ_ENOTLEADER).all()
                L.assert_rows(plain, L.model_lag(oras[r], followed, z), (r, "plain"))
                cur = {int(p): oras[r].state(int(p))["log_start_offset"] + CUR for p in followed}
                assert all(v > CUR for v in cur.values())  # retention has run on the follower
                want = L.model_lag(oras[r], followed, z, replica=True, cursor=cur)
                assert (want["status"] == A.RMQ_OK).all() and (want["records"] > 100).all()
                L.assert_rows(rep, want, (r, "replica"))
                allp = np.arange(len(views[r].gp), dtype=np.uint32)
                L.assert_rows(every, L.model_lag(oras[r], allp, np.zeros(len(allp)), 0, replica=True), (r, "every"))
        finally:
            for o in oras:
                o.close()
    finally:
        for e in engs:
            e.close()
        hub.close()


# ---- 7: the headroom on the engine
def _commit_mid(e) -> int:
    """Partition 0 of state 1: consumer 2 committed to a record in the middle of its retained log."""
    st = e.state(0)
    off = (st["log_start_offset"] + st["log_end_offset"]) // 2
    rc, s = e.commit_consumer_offset([0], [2], [off])
    assert rc == 0 and not s.any()
    return off


def _headroom_row(e):
    return _commit_mid(e), e.lag([0], [2])[0]


def test_headroom_on_the_engine(oracle_mod):
    cfg = U.cfg1()
    ora, _ = L.filled1(oracle_mod.OracleEngine)
    with ora:
        off = _commit_mid(ora)
        want = L.model_lag(ora, [0], [2])[0]
    h = int(want["headroom"])
    assert 32 <= h and h + 16 <= cfg.segment_bytes - cfg.index_interval, h
    e, _ = L.filled1(Engine)
    with e:
        got_off, row = _headroom_row(e)
        assert got_off == off and row == want
        first, second = (h // 32) * 16, h - (h // 32) * 16
        for k, sizes in enumerate(([first], [second - 16, 16] if second >= 32 else [second])):
            _, s = e.append(*L.bytes_batch(0, sizes, k))
            assert s["appended"] == len(sizes)
        rc, res, _, _ = e.fetch([0], [2], [1])
        assert (int(res["status"][0]), int(res["start_offset"][0]), int(res["count"][0])) == (A.RMQ_OK, off, 1)
        again = e.lag([0], [2])[0]
        assert int(again["status"]) == A.RMQ_OK and int(again["start_offset"]) == off
        assert int(again["start_pos"]) == int(want["start_pos"]) and int(again["end_pos"]) == int(want["end_pos"]) + h
    e, _ = L.filled1(Engine)
    with e:
        got_off, row = _headroom_row(e)
        assert row == want
        _, s = e.append(*L.bytes_batch(0, [h + 16], 9))
        assert s["appended"] == 1
        rc, res, _, _ = e.fetch([0], [2], [1])
        assert int(res["status"][0]) == A.RMQ_EOFFSET and int(res["start_offset"][0]) > off
        gone = e.lag([0], [2])[0]
        assert int(gone["status"]) == A.RMQ_EOFFSET and int(gone["evicted"]) == int(gone["start_offset"]) - off > 0


# ---- 8: ordering and flags
def test_ordering_and_flags(oracle_mod):
    e, cfg = L.filled1(Engine)
    ora, _ = L.filled1(oracle_mod.OracleEngine)
    with e, ora:
        hw0 = e.state(7)["high_watermark"]
        assert hw0 == 1
        o2 = ora.state(2)["log_start_offset"] + 3  # a retained record of partition 2
        batch = (np.full(3, 7, np.uint32), np.array([5, 0, 40], np.uint32), np.arange(45, dtype=np.uint8))
        tk, _ = e.append_async(*batch)  # not waited for: the group is still forming
        rc, st = e.commit_consumer_offset([7, 2], [1, 1], [1, o2])
        assert rc == 0 and not st.any()
        rows = e.lag([7, 2], [1, 1])  # no sync in between: ordered on the stream behind the commit
        assert rows["status"].tolist() == [A.RMQ_OK, A.RMQ_OK] and rows["start_offset"].tolist() == [1, o2]
        assert int(rows["records"][0]) in (0, 3)  # the lag call flushes nothing: the batch may not be applied yet
        ora.append(*batch), ora.commit_consumer_offset([7, 2], [1, 1], [1, o2])
        L.assert_rows(rows[1:], L.model_lag(ora, [2], [1]), "a partition the batch does not touch")
        e.sync()
        assert e.wait(tk)["appended"] == 3
        pidx, cons = np.array([7, 2, 7], np.uint32), np.array([1, 1, 0], np.uint32)
        want = L.model_lag(ora, pidx, cons)
        assert int(want["records"][0]) == 3
        L.assert_rows(e.lag(pidx, cons), want, "after sync")
        # RMQ_FETCH_COMMIT | RMQ_FETCH_VERIFY: accepted, nothing changes, nothing is committed
        snap = L.snapshot(e)
        L.assert_rows(e.lag(pidx, cons, flags=A.RMQ_FETCH_COMMIT | A.RMQ_FETCH_VERIFY), want, "commit | verify")
        L.assert_unchanged(e, snap)
        # an unknown bit in a host row: RMQ_EINVAL, nothing runs
        with pytest.raises(EngineError) as ei:
            e.lag(pidx, cons, flags=4)
        assert ei.value.status == A.RMQ_EINVAL
        req = L.reqs_array(pidx, cons)
        req[2, 3] = 0x40
        res = np.full(3 * 64, 0xEE, np.uint8)
        assert e.lib.rmq_lag(e.h, req.ctypes.data, None, 3, A.RMQ_MEM_HOST, res.ctypes.data) == A.RMQ_EINVAL
        assert (res == 0xEE).all()
        L.assert_unchanged(e, snap)
        # the profile region: one span per call
        e.profile(1)
        e.lag(pidx, cons), e.lag(pidx, cons)
        calls, ms = e.profile_query(10)
        e.profile(0)
        assert calls == 2 and ms > 0


# ---- 9: the wrappers
def test_wrappers(oracle_mod, tmp_path):
    cfg = dataclasses.replace(U.cfg1(), max_consumers=8)
    with Engine(cfg) as e:
        U.fill1(e)
        d = PartitionDirectory({"t": cfg.num_partitions}, max_consumers=8)
        broker = PartitionBroker(d, e)
        names = ["alpha", "beta", "gamma"]
        ids = [d.consumer(x) for x in names]
        e.commit_consumer_offset([0, 1, 2], ids, [3, 40, 50])
        groups = ["t-0", "t-1", "t-2", "t-3", "nosuch-0"]
        who = ["alpha", "beta", "gamma", "never-seen", "alpha"]
        rows = broker.consumer_lag(groups, who)
        direct = e.lag([0, 1, 2, 3, cfg.num_partitions], [ids[0], ids[1], ids[2], 0, ids[0]], offsets=[None, None, None, 0, None])
        L.assert_rows(rows, direct, "consumer_lag")
        assert rows["status"].tolist()[-1] == A.RMQ_ENOPART and (rows["status"][:4] != A.RMQ_ENOPART).all()
        assert int(rows["evicted"][3]) == e.state(3)["log_start_offset"] > 0
        # DurableLog.backlog: the replica cursor to the replica's commit
        parts = list(range(cfg.num_partitions))
        starts = [e.state(p)["log_start_offset"] for p in parts]
        log = DurableLog(e, str(tmp_path / "tier"), parts, 7, start=starts)
        try:
            back = log.backlog()
            direct = e.lag(np.array(parts, np.uint32), np.full(len(parts), 7, np.uint32), replica=True)
            assert back == {p: (int(direct["records"][p]), int(direct["bytes"][p])) for p in parts}
            assert sum(r for r, _ in back.values()) == sum(e.state(p)["high_watermark"] - starts[p] for p in parts) > 0
            assert log.spill() == sum(r for r, _ in back.values())
            assert log.backlog() == {p: (0, 0) for p in parts}
        finally:
            log.close()
