"""rmq_fetch_at on the GPU (FORMAT.md §7 "Explicit offsets"): every expected value is the model of
tests/fetch_at_util.py on the oracle (tests/test_fetch_at_model.py shows that the sweep here holds
every category it claims)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import fetch_at_util as F
import fetch_budget_util as B
import high_base_util as H
import scrub_util as U
from parity import run_ops
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine

pytestmark = pytest.mark.gpu

CAP = 1 << 19
NONE = F.NONE


@pytest.fixture(scope="module")
def ora1(oracle_mod):
    e, cfg = F.filled1(oracle_mod.OracleEngine)
    yield e, cfg
    e.close()


@pytest.fixture(scope="module")
def model1(ora1):
    return F.sweep1(ora1[0])  # computed once


@pytest.fixture(scope="module")
def clean():
    e, cfg = F.filled1(Engine)
    yield e, cfg
    e.close()


@pytest.fixture()
def fresh_pair(oracle_mod):
    e, cfg = F.filled1(Engine)
    o, _ = F.filled1(oracle_mod.OracleEngine)
    yield e, o, cfg
    e.close()
    o.close()


def _reqs(pidx, cons, mx, flags=0):
    req = np.zeros((len(pidx), 4), np.uint32)
    req[:, 0], req[:, 1], req[:, 2], req[:, 3] = pidx, cons, mx, flags
    return req


def _states(e):
    return [e.state(p) for p in range(e.cfg.num_partitions)]


# ---- 1: the sweep
@pytest.mark.parametrize("mx", F.SWEEP_MAX)
def test_sweep_on_state_1(clean, ora1, model1, mx):
    e, cfg = clean
    pidx, cons, offs = F.sweep_reqs1(ora1[0])
    want, cats = model1[mx]
    table, states, stats = F.tables(e), _states(e), e.replication_stats()
    F.assert_equals_model(e.fetch(pidx, cons, np.full(len(pidx), mx), offsets=offs), want, (mx, "sync host"))
    out = np.zeros(CAP, np.uint8)
    tk = e.fetch_async(None, None, None, out=out, req=_reqs(pidx, cons, mx), offsets=offs)
    rc, res, used = e.fetch_poll(tk, wait=True)
    F.assert_equals_model((rc, res, out, used), want, (mx, "async host"))
    assert np.array_equal(F.tables(e), table) and _states(e) == states  # nothing moved
    assert e.replication_stats() == stats


# ---- 2: workgroup and chunk edges of the LDS-staged offsets
def test_grid_edges_on_state_4(oracle_mod):
    cfg = F.cfg4()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        U.fill4(e), U.fill4(ora)
        for n in B.N4:
            pidx, cons, mx, offs = F.reqs4(n)
            want = F.model_fetch_at(ora, pidx, cons, mx, offs)
            F.assert_equals_model(e.fetch(pidx, cons, mx, offsets=offs), want, n)
        assert not F.tables(e).any()


# ---- 3: equivalences
@pytest.mark.parametrize("mx", (10, 0xFFFFFFFF))
def test_null_none_and_committed_offsets_change_nothing(clean, ora1, mx):
    e, cfg = clean
    pidx, cons = B.all_reqs1()
    n = len(pidx)
    for bud in (None, np.full(n, 512, np.uint32)):
        rc0, res0, b0, u0 = e.fetch(pidx, cons, np.full(n, mx), max_bytes=bud)  # rmq_fetch / rmq_fetch_bytes
        want = (ora1[0].fetch(pidx, cons, np.full(n, mx)) if bud is None else
                B.model_fetch(ora1[0], pidx, cons, mx, bud)[:4])
        F.assert_equals_model((rc0, res0, b0, u0), want, "plain")
        assert u0 > 0
        committed = np.array([e.consumer_offsets(int(p))[int(c)] for p, c in zip(pidx, cons)], np.uint64)
        for what, offs in (("null", None), ("none", np.full(n, NONE, np.uint64)), ("committed", committed)):
            for asyn in (False, True):
                req, res, out, used = _reqs(pidx, cons, mx), np.zeros(n, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8), C.c_uint64()
                args = (e.h, req.ctypes.data, None if offs is None else offs.ctypes.data,
                        None if bud is None else bud.ctypes.data, n, A.RMQ_MEM_HOST, out.ctypes.data, CAP, res.ctypes.data)
                if asyn:
                    t = C.c_uint64()
                    assert e.lib.rmq_fetch_at_async(*args, C.byref(t)) == A.RMQ_OK
                    rc = e.lib.rmq_fetch_poll(e.h, t.value, 1, C.byref(used))
                else:
                    rc = e.lib.rmq_fetch_at(*args, C.byref(used))
                assert (rc, used.value) == (rc0, u0) and np.array_equal(res, res0), (what, asyn)
                assert np.array_equal(out[:u0], b0[:u0]) and not out[u0:].any(), (what, asyn)
    # the Python entry points: a scalar, None entries
    got = e.fetch(pidx, cons, np.full(n, mx), offsets=[None] * n)
    F.assert_equals_model(got, ora1[0].fetch(pidx, cons, np.full(n, mx)), "None entries")
    assert e.lib.rmq_fetch_at(e.h, None, None, None, 1, A.RMQ_MEM_HOST, None, 0, None, None) == A.RMQ_EINVAL
    assert e.lib.rmq_fetch_at(e.h, _reqs(pidx, cons, mx).ctypes.data, None, None, n, 7, None, 0,
                              np.zeros(n, FETCH_RES_DTYPE).ctypes.data, None) == A.RMQ_EINVAL


# ---- 4: flags
def test_commit_is_a_seek_and_a_read(fresh_pair):
    e, ora, cfg = fresh_pair
    lo = [ora.state(p)["log_start_offset"] for p in range(F.P1)]
    pidx, cons = np.array([2, 3, 4, 5, 2]), np.array([1, 1, 1, 2, 3])
    offs = np.array([lo[2] + 3, lo[3] - 1, NONE, 2 ** 32 + 5, lo[2] + 3], np.uint64)
    want = F.model_fetch_at(ora, pidx, cons, 5, offs, commit=True)
    assert [int(x) for x in want[1]["status"]] == [A.RMQ_OK, A.RMQ_EOFFSET, A.RMQ_OK, A.RMQ_OK, A.RMQ_OK]
    stats = e.replication_stats()
    F.assert_equals_model(e.fetch(pidx, cons, np.full(5, 5), commit=True, offsets=offs), want)
    assert np.array_equal(F.tables(e), F.tables(ora))
    assert int(e.consumer_offsets(2)[1]) == lo[2] + 8 and int(e.consumer_offsets(5)[2]) == 2 ** 32 + 5
    assert e.replication_stats() == stats  # (no transport: no round)
    # a plain fetch reads on from there
    allp, allc = B.all_reqs1()
    rc, res, out, used = got = e.fetch(allp, allc, np.full(len(allp), 10))
    F.assert_equals_model(got, ora.fetch(allp, allc, np.full(len(allp), 10)), "reads on")
    assert int(res["start_offset"][2 * F.NC1 + 1]) == lo[2] + 8
    # two committing requests of one (partition, consumer): refused as ever, nothing launched
    table = F.tables(e)
    with pytest.raises(Exception) as ex:
        e.fetch(np.array([2, 2]), np.array([1, 1]), np.full(2, 5), out=np.zeros(4096, np.uint8), commit=True,
                offsets=np.array([lo[2], lo[2] + 1], np.uint64))
    assert ex.value.status == A.RMQ_EINVAL
    assert np.array_equal(F.tables(e), table)


def test_verify_refuses_a_flipped_record_of_an_addressed_slice(fresh_pair):
    e, ora, cfg = fresh_pair
    S = cfg.segment_bytes
    recs = U.host_walk(e, cfg, 0, 3)[2]
    k = next(i for i in range(2, 7) if recs[i][2] > 0)
    pidx, cons = np.array([3, 2]), np.array([0, 0])
    offs = np.array([recs[2][0], ora.state(2)["log_start_offset"] + 4], np.uint64)
    table = F.tables(e)
    clean_want = F.model_fetch_at(ora, pidx, cons, 5, offs)
    F.assert_equals_model(e.fetch(pidx, cons, np.full(2, 5), verify=True, offsets=offs), clean_want, "clean")
    e.fault_flip_ring(0, 3, (recs[k][1] + 16) % S)
    want = F.model_fetch_at(ora, pidx, cons, 5, offs, commit=True)
    rc, res, out, used = e.fetch(pidx, cons, np.full(2, 5), commit=True, verify=True, offsets=offs)
    assert (rc, used) == (want[0], want[3])
    assert (int(res["status"][0]), int(res["count"][0])) == (A.RMQ_ECORRUPT, 0)
    assert all(int(res[f][0]) == int(want[1][f][0]) for f in ("start_offset", "out_pos", "bytes"))
    assert res[1] == want[1][1]  # the other partition: served, and committed
    lo = int(res["out_pos"][1])
    assert np.array_equal(out[lo:lo + int(res["bytes"][1])], want[2][lo:lo + int(res["bytes"][1])])
    table[2, 0] = int(offs[1]) + 5
    assert np.array_equal(F.tables(e), table)  # the refused request committed nothing


def test_replica_reads_at_an_offset_leave_the_cursor(fresh_pair):
    e, ora, cfg = fresh_pair
    pidx, cons = np.arange(F.P1), np.zeros(F.P1, np.uint32)
    starts = np.array([ora.state(p)["log_start_offset"] for p in range(F.P1)], np.uint64)
    for x in (e, ora):
        x.set_replica_cursor(pidx, starts)
    st = [ora.state(p) for p in range(F.P1)]
    offs = np.array([starts[0] + 2, starts[1] - 1, NONE, st[3]["high_watermark"], st[4]["high_watermark"] - 1,
                     2 ** 32 + 5, NONE, 0], np.uint64)

    def cursors(x):
        return [int(v) for v in x.fetch(pidx, cons, np.zeros(F.P1), replica=True)[1]["start_offset"]]

    table = F.tables(e)
    want = F.model_fetch_at(ora, pidx, cons, 6, offs, replica=True)
    assert A.RMQ_EOFFSET in want[1]["status"] and want[3] > 0
    F.assert_equals_model(e.fetch(pidx, cons, np.full(F.P1, 6), replica=True, offsets=offs), want, "no commit")
    assert cursors(e) == cursors(ora) == [int(v) for v in starts]
    want = F.model_fetch_at(ora, pidx, cons, 6, offs, commit=True, replica=True)
    F.assert_equals_model(e.fetch(pidx, cons, np.full(F.P1, 6), commit=True, replica=True, offsets=offs), want, "commit")
    assert cursors(e) == cursors(ora) and cursors(e)[0] == int(starts[0]) + 8
    assert np.array_equal(F.tables(e), table)  # the consumer table is not the replica cursor


# ---- 5: budgets and explicit offsets together
def test_budgets_and_offsets_on_state_3(oracle_mod):
    cfg = dataclasses.replace(U.cfg3(), max_consumers=F.SCRATCH0 + B.NC3)
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        U.fill3(e), U.fill3(ora)
        lo = ora.state(B.P3)["log_start_offset"]
        pidx, cons = np.full(B.NC3, B.P3), np.arange(B.NC3) % 4
        offs, mx = lo + np.arange(B.NC3, dtype=np.uint64), np.full(B.NC3, 0xFFFFFFFF)
        for bud in (144, 1000, 4096):
            want = F.model_fetch_at(ora, pidx, cons, mx, offs, max_bytes=bud)
            F.assert_equals_model(e.fetch(pidx, cons, mx, max_bytes=bud, offsets=offs), want, bud)
            assert (want[1]["status"] == A.RMQ_ENOSPC).any() and (want[1]["count"] > 0).any()
        assert not F.tables(e).any()


# ---- 6: read-ahead
def test_read_ahead_of_four_tickets(clean, ora1):
    e, cfg = clean
    p, c, k = 3, 0, 4
    o = int(e.consumer_offsets(p)[c])
    _, res0, b0, u0 = e.fetch([p], [c], [4 * k])
    assert int(res0["count"][0]) == 4 * k and int(res0["start_offset"][0]) == o
    outs = [np.zeros(1 << 14, np.uint8) for _ in range(5)]
    tks = [e.fetch_async([p], [c], [k], out=outs[i], offsets=[o + i * k]) for i in range(4)]
    assert int(e.consumer_offsets(p)[c]) == o
    tks.append(e.fetch_async([p], [c], [k], out=outs[4], offsets=[o]))  # a fifth completes the oldest
    first = e.fetch_poll(tks[0])
    assert first is not None
    got = [first] + [e.fetch_poll(t, wait=True) for t in tks[1:]]
    cat = b""
    for i in range(4):
        rc, res, used = got[i]
        want = F.model_fetch_at(ora1[0], [p], [c], [k], [o + i * k])
        F.assert_equals_model((rc, res, outs[i], used), want, i)
        assert int(res["count"][0]) == k
        cat += outs[i][:used].tobytes()
    assert cat == b0[:u0].tobytes()
    assert np.array_equal(outs[4][:got[4][2]], outs[0][:got[0][2]])
    assert int(e.consumer_offsets(p)[c]) == o


# ---- 7: the commit behind the log end
def test_offsets_between_the_high_watermark_and_the_log_end(oracle_mod):
    cfg = F.cfg1()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        lens = np.array([5, 40, 0, 17, 100, 16, 1, 33, 64, 7, 250, 3, 90, 12, 48, 9, 31, 2, 77, 20], np.uint32)
        payload = np.arange(int(lens.sum()), dtype=np.uint32).astype(np.uint8)
        for x in (e, ora):
            x.set_replicas(5, [0, 1, 2], 0)  # two slots on other ranks: nothing commits without their acks
            x.append(np.full(20, 5, np.uint32), lens, payload)
            x.ack([5], [1], [12])
        st = ora.state(5)
        assert e.state(5) == st and (st["high_watermark"], st["log_end_offset"]) == (12, 20)
        offs = np.array([10, 11, 12, 13, 16, 19, 20, 21], np.uint64)
        pidx, cons = np.full(8, 5), np.arange(8) % 4
        for mx in (1, 10, 0xFFFFFFFF):
            want = F.model_fetch_at(ora, pidx, cons, mx, offs)
            assert not want[1]["status"].any() and not want[1]["count"][2:].any() and want[1]["count"][:2].all()
            assert np.array_equal(want[1]["start_offset"], offs)
            F.assert_equals_model(e.fetch(pidx, cons, np.full(8, mx), offsets=offs), want, mx)


# ---- 8: row kinds
def test_pinned_and_device_rows(clean, ora1, model1):
    e, cfg = clean
    pidx, cons, offs = F.sweep_reqs1(ora1[0])
    n, mx = len(pidx), 10
    want = model1[mx][0]
    d_out, d_req, d_res, d_at = e.device_alloc(CAP), e.device_alloc(16 * n), e.device_alloc(32 * n), e.device_alloc(8 * n + 8)
    try:
        req, res = e.fetch_rows(n)
        req[:] = _reqs(pidx, cons, mx)
        for asyn in (False, True):
            e.h2d(d_out, np.zeros(CAP, np.uint8))
            res[:] = np.zeros(1, FETCH_RES_DTYPE)[0]
            if asyn:
                tk = e.fetch_async(None, None, None, d_out=d_out, out_cap=CAP, req=req, res=res, pinned_rows=True, offsets=offs)
                rc, r, used = e.fetch_poll(tk, wait=True)
            else:
                rc, r, used = e.fetch_device(None, None, None, d_out, CAP, req=req, res=res, pinned_rows=True, offsets=offs)
            got = np.empty(CAP, np.uint8)
            e.d2h(got, d_out)
            F.assert_equals_model((rc, r.copy(), got, used), want, ("page-locked rows", asyn))
        e.host_release(req), e.host_release(res)
        # device rows, device offsets
        e.h2d(d_req, _reqs(pidx, cons, mx).view(np.uint8).reshape(-1))
        e.h2d(d_at, offs.view(np.uint8))
        e.h2d(d_out, np.zeros(CAP, np.uint8))
        rc, _, used = e.fetch_device(None, None, None, d_out, CAP, d_rows=(n, d_req, d_res), offsets=d_at)
        res, got = np.zeros(n, FETCH_RES_DTYPE), np.empty(CAP, np.uint8)
        e.d2h(res.view(np.uint8), d_res), e.d2h(got, d_out)
        F.assert_equals_model((rc, res, got, used), want, "device rows")
        # with a device budget array too
        d_bud = e.device_alloc(4 * n)
        try:
            e.h2d(d_bud, np.full(n, 512, np.uint32).view(np.uint8))
            e.h2d(d_out, np.zeros(CAP, np.uint8))
            rc, _, used = e.fetch_device(None, None, None, d_out, CAP, d_rows=(n, d_req, d_res, d_bud), offsets=d_at)
            e.d2h(res.view(np.uint8), d_res), e.d2h(got, d_out)
            F.assert_equals_model((rc, res, got, used), F.model_fetch_at(ora1[0], pidx, cons, mx, offs, max_bytes=512),
                                  "device rows, budgets")
        finally:
            e.device_free(d_bud)
        # misaligned device offsets: refused on the host, nothing launched
        e.h2d(d_res, np.full(32 * n, 0xEE, np.uint8))
        used = C.c_uint64(7)
        assert e.lib.rmq_fetch_at(e.h, C.c_void_p(d_req), C.c_void_p(d_at + 4), None, n,
                                  A.RMQ_MEM_DEVICE | A.RMQ_FETCH_DEVICE_ROWS, C.c_void_p(d_out), CAP, C.c_void_p(d_res),
                                  C.byref(used)) == A.RMQ_EINVAL
        rows = np.zeros(32 * n, np.uint8)
        e.d2h(rows, d_res)
        assert (rows == 0xEE).all() and used.value == 0
    finally:
        for d in (d_out, d_req, d_res, d_at):
            e.device_free(d)


@pytest.mark.parametrize("dma_in", ["0", "1"])
def test_rows_by_dma(monkeypatch, ora1, model1, dma_in):
    monkeypatch.setenv("RMQ_FETCH_DMA", "2")
    monkeypatch.setenv("RMQ_FETCH_DMA_IN", dma_in)
    e, cfg = F.filled1(Engine)
    try:
        pidx, cons, offs = F.sweep_reqs1(ora1[0])
        F.assert_equals_model(e.fetch(pidx, cons, np.full(len(pidx), 10), offsets=offs), model1[10][0])
    finally:
        e.close()


def test_profile_replay_is_idempotent(ora1, model1):
    e, cfg = F.filled1(Engine)
    try:
        e.profile(3)
        pidx, cons, offs = F.sweep_reqs1(ora1[0])
        table = F.tables(e)
        for _ in range(2):
            F.assert_equals_model(e.fetch(pidx, cons, np.full(len(pidx), 10), offsets=offs), model1[10][0])
        assert np.array_equal(F.tables(e), table)
    finally:
        e.close()


# ---- 9: bases past 2^32 and 2^53
def test_high_bases(oracle_mod):
    cfg = H.cfg_high(max_consumers=F.SCRATCH0 + 8)
    bases = {p: b for p, b in H.bases_for(cfg.index_interval).items() if p in (0, 2, 4)}
    assert bases[2][0] > 2 ** 32 and bases[4][0] > 2 ** 53
    with Engine(cfg) as e, H.Translated(oracle_mod.OracleEngine(cfg), cfg, bases) as t:
        H.rebase(e, bases, t)
        run_ops(e, t, cfg, [("append", H.first_batch())] + [("append", b) for b in H.scenario_batches(2)], check=False)
        pidx, cons, offs = [], [], []
        for p in (2, 4, 0):
            st = t.state(p)
            lo, hw = st["log_start_offset"], st["high_watermark"]
            assert e.state(p)["log_start_offset"] == lo and hw - lo > 40 and lo >= bases[p][0]
            for k in (0, 1, 17, hw - lo - 1, hw - lo, hw - lo + 1, 2 ** 32):
                pidx.append(p), cons.append(len(offs) % 4), offs.append(lo + k)
            pidx.append(p), cons.append(0), offs.append(NONE)
        pidx, cons, offs = np.array(pidx), np.array(cons), np.array(offs, np.uint64)
        table = F.tables(e)
        for mx in (1, 10, 0xFFFFFFFF):
            want = F.model_fetch_at(t, pidx, cons, np.full(len(pidx), mx), offs)
            assert (want[1]["start_offset"][offs != NONE] == offs[offs != NONE]).all()
            F.assert_equals_model(e.fetch(pidx, cons, np.full(len(pidx), mx), offsets=offs), want, mx)
        assert np.array_equal(F.tables(e), table)
