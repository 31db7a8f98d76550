"""RMQ_FETCH_FILL on the GPU (FORMAT.md §7 "Filling a bounded output"): every expected value is the
model of tests/fetch_fill_util.py on the oracle (tests/test_fetch_fill_model.py shows that each
sweep here holds every category it claims). Every comparison is whole rows, the output bytes of the
served ranges, bytes_used and the return code, and after a committing call the consumer table or the
replica cursors against the oracle's."""
import glob
import os

import numpy as np
import pytest

import fetch_at_util as FA
import fetch_budget_util as B
import fetch_fill_util as F
import scrub_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd import tier as T
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, EngineError

pytestmark = pytest.mark.gpu

CAP = 1 << 17
N1 = B.P1 * B.NC1
PIDX1, CONS1 = B.all_reqs1()


@pytest.fixture(scope="module")
def ora1(oracle_mod):
    e, cfg = B.filled1(oracle_mod.OracleEngine)
    yield e, cfg
    e.close()


@pytest.fixture(scope="module")
def model1(ora1):
    return F.sweep1(ora1[0])  # computed once, read by every test that sweeps state 1


@pytest.fixture(scope="module")
def clean():
    e, cfg = B.filled1(Engine)
    yield e, cfg
    e.close()


@pytest.fixture()
def fresh_pair(oracle_mod):
    e, cfg = B.filled1(Engine)
    o, _ = B.filled1(oracle_mod.OracleEngine)
    yield e, o, cfg
    e.close()
    o.close()


def _reqs(mx, flags=0, pidx=PIDX1, cons=CONS1):
    req = np.zeros((len(pidx), 4), np.uint32)
    req[:, 0], req[:, 1], req[:, 2], req[:, 3] = pidx, cons, mx, flags
    return req


def _tables(e):
    return np.stack([e.consumer_offsets(p) for p in range(e.cfg.num_partitions)])


def _cursors(e, parts):
    """The replica cursors (an empty replica read starts at the cursor)."""
    _, res, _, _ = e.fetch(np.asarray(parts), np.zeros(len(parts), np.uint32), np.zeros(len(parts), np.uint32), replica=True)
    assert (res["status"] == A.RMQ_OK).all()
    return [int(x) for x in res["start_offset"]]


@pytest.mark.parametrize("mx", F.SWEEP_MAX)
def test_sweep_on_state_1_host_rows(clean, model1, mx):
    e, cfg = clean
    full, models = model1[mx]
    for cap, want in models.items():
        got = e.fetch(PIDX1, CONS1, np.full(N1, mx), out_cap=cap, fill=True)
        F.assert_equals_model(got, want, (mx, cap, "ordinary rows, host output"))


@pytest.mark.parametrize("mx", F.SWEEP_MAX)
def test_sweep_on_state_1_device_rows(clean, model1, mx):
    e, cfg = clean
    full, models = model1[mx]
    d_out, d_req, d_res = e.device_alloc(CAP), e.device_alloc(16 * N1), e.device_alloc(32 * N1)
    try:
        e.h2d(d_req, _reqs(mx).view(np.uint8).reshape(-1))
        e.h2d(d_out, np.zeros(CAP, np.uint8))
        for cap, want in models.items():
            assert cap <= CAP
            rc, _, used = e.fetch_device(None, None, None, d_out, cap, d_rows=(N1, d_req, d_res), fill=True)
            res, got = np.zeros(N1, FETCH_RES_DTYPE), np.zeros(max(used, 16), np.uint8)
            e.d2h(res.view(np.uint8), d_res), e.d2h(got, d_out)
            F.assert_equals_model((rc, res, got, used), want, (mx, cap, "device rows, device output"))
    finally:
        for d in (d_out, d_req, d_res):
            e.device_free(d)


@pytest.mark.parametrize("mx", F.SWEEP_MAX)
def test_sweep_on_state_1_commit(fresh_pair, model1, mx):
    e, ora, cfg = fresh_pair
    full, models = model1[mx]
    tab0 = _tables(ora)
    assert np.array_equal(_tables(e), tab0)
    back = (PIDX1.astype(np.uint32), CONS1.astype(np.uint32), tab0[PIDX1, CONS1].astype(np.uint64))
    for cap, plain in models.items():
        want = F.model_fill(ora, PIDX1, CONS1, mx, None, cap, commit=True, full=full)
        assert np.array_equal(want[1], plain[1])  # (committing changes no row)
        got = e.fetch(PIDX1, CONS1, np.full(N1, mx), out_cap=cap, commit=True, fill=True)
        F.assert_equals_model(got, want, (mx, cap, "commit"))
        te, to = _tables(e), _tables(ora)
        assert np.array_equal(te, to), (mx, cap)
        moved = (want[1]["status"] == A.RMQ_OK) & (want[1]["count"] > 0)
        assert (te != tab0).sum() == moved.sum()  # pending and cut-to-nothing rows committed nothing
        for x in (e, ora):
            rc, st = x.commit_consumer_offset(*back)
            assert rc == 0 and not st.any()


@pytest.mark.parametrize("mx", F.SWEEP_MAX)
def test_sweep_on_state_1_verify(clean, model1, mx):
    e, cfg = clean
    full, models = model1[mx]
    for cap, want in models.items():
        got = e.fetch(PIDX1, CONS1, np.full(N1, mx), out_cap=cap, verify=True, fill=True)
        F.assert_equals_model(got, want, (mx, cap, "verify, clean log"))
    # the position cache after pending and cut rows: the plain unbounded fetch is still the oracle's
    rc, res, out, used = e.fetch(PIDX1, CONS1, np.full(N1, mx))
    assert (rc, used) == (full[0], full[3]) and np.array_equal(res, full[1]) and np.array_equal(out[:used], full[2][:used])


def test_verify_refuses_a_flip_inside_the_cut(fresh_pair):
    e, ora, cfg = fresh_pair
    S = cfg.segment_bytes
    # consumer 0 of partitions 3 and 2 stands at the log start: 12 records asked of each, the
    # output ends 8 bytes after the fourth record of the second
    pidx, cons, mx = np.array([3, 2]), np.array([0, 0]), np.full(2, 12)
    recs = U.host_walk(e, cfg, 0, 2)[2][:12]
    size = lambda x: 16 + ((x[2] + 15) & ~15)  # noqa: E731
    full = F.unbounded(ora, pidx, cons, mx)
    cap = int(full[1]["bytes"][0]) + sum(size(x) for x in recs[:4]) + 8
    want = F.model_fill(ora, pidx, cons, mx, None, cap, commit=True, full=full)
    assert want[4] == ["whole", "cut_mid"] and int(want[1]["count"][1]) == 4
    inside = next(x for x in recs[:4] if x[2] > 0)  # a payload byte of the cut slice
    e.fault_flip_ring(0, 2, (inside[1] + 16) % S)
    before = e.consumer_offsets(2).copy()
    rc, res, out, used = e.fetch(pidx, cons, mx, out_cap=cap, commit=True, verify=True, fill=True)
    assert (rc, used) == (want[0], want[3])
    assert res[0] == want[1][0]
    assert (int(res["status"][1]), int(res["count"][1])) == (A.RMQ_ECORRUPT, 0)
    assert all(int(res[f][1]) == int(want[1][f][1]) for f in ("start_offset", "out_pos", "bytes", "reserved"))
    assert np.array_equal(e.consumer_offsets(2), before)  # refused: nothing committed
    assert np.array_equal(e.consumer_offsets(3), ora.consumer_offsets(3))  # the whole one is


@pytest.mark.parametrize("budgets", [False, True])
def test_grid_and_chunk_edges_on_state_4(oracle_mod, budgets):
    cfg = U.cfg4()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        U.fill4(e), U.fill4(ora)
        for n in B.N4:
            for rstar, shift, cap, full in F.calls4(ora, n, budgets):
                pidx, cons, mx, bud = F.reqs4(n, shift, budgets)
                want = F.model_fill(ora, pidx, cons, mx, bud, cap, full=full)
                got = e.fetch(pidx, cons, mx, out_cap=cap, max_bytes=bud, fill=True)
                F.assert_equals_model(got, want, (n, rstar, shift, cap))


def test_cut_point_edges_on_state_3(oracle_mod):
    e, cfg = B.filled3(Engine)
    ora, _ = B.filled3(oracle_mod.OracleEngine)
    try:
        pidx, cons, mx, full, j, caps = F.edge_calls3(ora, cfg)
        for k, cap in enumerate(caps):
            want = F.model_fill(ora, pidx, cons, mx, None, cap, full=full)
            F.assert_equals_model(e.fetch(pidx, cons, mx, out_cap=cap, fill=True), want, (k, j, cap))
    finally:
        e.close()
        ora.close()


def test_offsets_budgets_and_fill_in_one_call(oracle_mod):
    e, cfg = FA.filled1(Engine)
    ora, _ = FA.filled1(oracle_mod.OracleEngine)
    try:
        pidx, cons, offs = FA.sweep_reqs1(ora)
        n = len(pidx)
        bud = np.array((0, 272, 512, 1520), np.uint64)[np.arange(n) % 4]
        full = F.unbounded(ora, pidx, cons, 10, bud, offsets=offs)
        P = F.prefix(full[1])
        crossed = set()
        for cap in (int(P[n]) // 3 + 8, int(P[n]) // 2 & ~15, int(P[n]) - 16):
            want = F.model_fill(ora, pidx, cons, 10, bud, cap, offsets=offs, full=full)
            crossed |= set(want[4])
            got = e.fetch(pidx, cons, np.full(n, 10), out_cap=cap, max_bytes=bud, offsets=offs, fill=True)
            F.assert_equals_model(got, want, cap)
        assert {"whole", "pending", "passthrough"} <= crossed and any(c.startswith("cut") for c in crossed)
        assert np.array_equal(FA.tables(e), FA.tables(ora))  # nothing committed, nothing moved
    finally:
        e.close()
        ora.close()


def test_async_burst_of_filling_tickets(clean, model1):
    """Four filling tickets with an ordinary one between them, each answered as its synchronous twin."""
    e, cfg = clean
    full, models = model1[10]
    caps = [c for c, m in models.items() if c >= 16 and any(x.startswith("cut") for x in m[4])]
    caps = [caps[0], caps[len(caps) // 3], caps[len(caps) // 2], caps[-1]]
    outs = [np.zeros(CAP, np.uint8) for _ in range(5)]
    tks = []
    for k in range(5):
        if k == 2:  # the ordinary one
            tks.append(e.fetch_async(None, None, None, out=outs[k], req=_reqs(10)))
        else:
            c = caps[k - (k > 2)]
            tks.append(e.fetch_async(None, None, None, out=outs[k], out_cap=c, req=_reqs(10), fill=True))
    for k, tk in enumerate(tks):
        rc, res, used = e.fetch_poll(tk, wait=True)
        if k == 2:
            assert (rc, used) == (full[0], full[3]) and np.array_equal(res, full[1])
            assert np.array_equal(outs[k][:used], full[2][:used])
        else:
            c = caps[k - (k > 2)]
            F.assert_equals_model((rc, res, outs[k], used), models[c], (k, c))
            assert not outs[k][used:].any()  # nothing written past what was served


def test_pinned_rows_and_the_profiler(clean, model1):
    """Page-locked rows into a device output, synchronous and asynchronous; and under the profiler a
    filling call runs once however many replays are asked for."""
    e, cfg = clean
    full, models = model1[1024]
    caps = [c for c, m in models.items() if c >= 16 and any(x.startswith("cut") for x in m[4])]
    d_out = e.device_alloc(CAP)
    req, res = e.fetch_rows(N1)
    try:
        req[:] = _reqs(1024)
        for k, cap in enumerate(caps[::7]):
            e.h2d(d_out, np.zeros(CAP, np.uint8))
            if k % 2:
                tk = e.fetch_async(None, None, None, d_out=d_out, out_cap=cap, req=req, res=res, pinned_rows=True, fill=True)
                rc, r, used = e.fetch_poll(tk, wait=True)
            else:
                rc, r, used = e.fetch_device(None, None, None, d_out, cap, req=req, res=res, pinned_rows=True, fill=True)
            got = np.empty(CAP, np.uint8)
            e.d2h(got, d_out)
            F.assert_equals_model((rc, r.copy(), got, used), models[cap], (cap, "page-locked rows"))
            assert not got[used:].any()
        cap = caps[len(caps) // 2]
        e.profile(8)
        rc, r, used = e.fetch_device(None, None, None, d_out, cap, req=req, res=res, pinned_rows=True, fill=True)
        runs, ms = e.profile_query(4)
        spans, _ = e.profile_query(3)
        e.profile(0)
        assert (runs, spans) == (1, 0) and ms > 0
        got = np.empty(CAP, np.uint8)
        e.d2h(got, d_out)
        F.assert_equals_model((rc, r.copy(), got, used), models[cap], (cap, "profiled"))
    finally:
        e.host_release(req), e.host_release(res)
        e.device_free(d_out)


def test_replica_commit_leaves_pending_cursors(fresh_pair):
    e, ora, cfg = fresh_pair
    parts = np.arange(B.P1)
    cons, mx = np.zeros(B.P1, np.uint32), np.full(B.P1, 1024)
    starts = [e.state(int(p))["log_start_offset"] for p in parts]
    for x in (e, ora):
        x.set_replica_cursor(parts, starts)
    full = F.unbounded(ora, parts, cons, mx, replica=True)
    cap = (full[3] // 2 & ~15) + 8
    want = F.model_fill(ora, parts, cons, mx, None, cap, commit=True, replica=True, full=full)
    assert "pending" in want[4] and "whole" in want[4] and any(c.startswith("cut") for c in want[4])
    got = e.fetch(parts, cons, mx, out_cap=cap, commit=True, replica=True, fill=True)
    F.assert_equals_model(got, want, cap)
    cur = _cursors(e, parts)
    assert cur == _cursors(ora, parts)
    for r, c in enumerate(want[4]):
        if c == "pending":
            assert cur[r] == starts[r]  # put off: the cursor did not move
        elif c == "whole" and int(want[1]["count"][r]):
            assert cur[r] == starts[r] + int(want[1]["count"][r])


@pytest.mark.parametrize("mx", F.SWEEP_MAX)
def test_a_call_that_fits_is_the_call_without_the_flag(clean, model1, mx):
    e, cfg = clean
    full = model1[mx][0]
    for cap in (full[3], full[3] + 16, CAP):
        rc0, res0, out0, used0 = e.fetch(PIDX1, CONS1, np.full(N1, mx), out_cap=cap)
        rc1, res1, out1, used1 = e.fetch(PIDX1, CONS1, np.full(N1, mx), out_cap=cap, fill=True)
        assert (rc0, used0) == (rc1, used1) == (A.RMQ_OK, full[3])
        assert np.array_equal(res0, res1) and np.array_equal(out0, out1) and np.array_equal(res1, full[1])
    # the size probe: no output at all names the first record to make room for
    import ctypes as C
    req, res, used = _reqs(mx), np.zeros(N1, FETCH_RES_DTYPE), C.c_uint64()
    rc = e.lib.rmq_fetch(e.h, req.ctypes.data, N1, A.RMQ_MEM_HOST | A.RMQ_FETCH_FILL, None, 0, res.ctypes.data, C.byref(used))
    want = model1[mx][1][0]
    assert (rc, used.value) == (A.RMQ_OK, 0) and np.array_equal(res, want[1]) and "cut_zero_enospc" in want[4]


def _segment_files(root):
    out = {}
    for path in sorted(glob.glob(os.path.join(root, "**", "*" + T.SEG_SUFFIX), recursive=True)):
        with open(path, "rb") as f:
            out[os.path.relpath(path, root)] = f.read()
    return out


def test_filling_spill_on_a_zipf_backlog(tmp_path, oracle_mod):
    """DurableLog(spill_bytes=N, fill=True) on a skewed backlog: the files of the unbounded spill,
    every pass but the last full to within one record, and no more passes than the equal shares."""
    NP, N = 64, 1 << 15
    cfg = U.cfg1(num_partitions=NP, segment_bytes=1 << 19, max_batch_records=4096, max_batch_bytes=1 << 20)
    parts = range(NP)
    rng = np.random.default_rng(7)
    pidx = np.minimum(rng.zipf(1.3, 3000) - 1, NP - 1).astype(np.uint32)
    lens = rng.integers(1, 400, pidx.size).astype(np.uint32)
    payload = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    s_max = 16 + ((int(lens.max()) + 15) & ~15)
    backlog = int((16 + ((lens.astype(np.int64) + 15) & ~15)).sum())
    assert backlog > 8 * N and np.bincount(pidx, minlength=NP)[0] > pidx.size // 5  # skewed, many passes

    def filled():
        e = Engine(cfg)
        _, st = e.append(pidx, lens, payload)
        assert st["appended"] == pidx.size, st
        return e

    with pytest.raises(ValueError):  # the oracle's fetch does not fill
        with oracle_mod.OracleEngine(cfg) as o:
            T.DurableLog(o, str(tmp_path / "o"), parts, 0, spill_bytes=N, fill=True)
    files, passes, used = {}, {}, {}
    for name, kw in (("ref", {}), ("share", dict(spill_bytes=N)), ("fill", dict(spill_bytes=N, fill=True))):
        e = filled()
        try:
            log = T.DurableLog(e, str(tmp_path / name), parts, 0, **kw)
            assert log.spill() == pidx.size
            log.close()
            files[name], passes[name], used[name] = _segment_files(str(tmp_path / name)), log.passes, log.pass_bytes
            if kw:
                assert log._buf.size <= N
        finally:
            e.close()
    print("passes:", passes, "bytes per filling pass:", used["fill"])
    assert files["fill"] == files["ref"] == files["share"] and len(files["ref"]) > 1
    # (the passes end with one that moves nothing; of those that moved records the last takes the rest)
    moving = [u for u in used["fill"] if u]
    assert all(u > N - s_max for u in moving[:-1]) and all(u <= N for u in moving) and len(moving) > 8
    assert sum(used["fill"]) == backlog
    assert passes["fill"] <= passes["share"]


def test_filling_spill_names_a_record_larger_than_the_buffer(tmp_path, oracle_mod):
    cfg = U.cfg3()
    parts = range(U.PARTS3)
    with oracle_mod.OracleEngine(cfg) as o:
        U.fill3(o)
        sizes = B.sizes3(o, cfg)
    assert int(sizes[0]) == 8224
    e = Engine(cfg)
    try:
        U.fill3(e)
        starts = np.array([e.state(p)["log_start_offset"] for p in parts], np.int64)
        small = T.DurableLog(e, str(tmp_path / "small"), parts, 0, start=starts, spill_bytes=4096, fill=True)
        with pytest.raises(EngineError) as ex:
            small.spill()
        assert ex.value.status == A.RMQ_ENOSPC and "8224" in str(ex.value), str(ex.value)
        small.close()
        assert not any(_segment_files(str(tmp_path / "small")).values())
        assert _cursors(e, list(parts)) == [int(s) for s in starts]  # nothing moved
    finally:
        e.close()
