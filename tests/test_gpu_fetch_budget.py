"""rmq_fetch_bytes on the GPU (FORMAT.md §7 "Byte budgets"): every expected value is the model of
tests/fetch_budget_util.py on the oracle (tests/test_fetch_budget_model.py shows that each sweep
here holds every category it claims)."""
import glob
import os

import numpy as np
import pytest

import fetch_budget_util as B
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
    return B.sweep1(ora1[0])  # computed once, read by every test that sweeps state 1


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


def _device_call(e, d_out, req, res, asyn, pinned, max_bytes):
    e.h2d(d_out, np.zeros(CAP, np.uint8))
    res[:] = np.zeros(1, FETCH_RES_DTYPE)[0]
    if asyn:
        tk = e.fetch_async(None, None, None, d_out=d_out, out_cap=CAP, req=req, res=res, pinned_rows=pinned,
                           max_bytes=max_bytes)
        rc, r, used = e.fetch_poll(tk, wait=True)
    else:
        rc, r, used = e.fetch_device(None, None, None, d_out, CAP, req=req, res=res, pinned_rows=pinned,
                                     max_bytes=max_bytes)
    got = np.empty(CAP, np.uint8)
    e.d2h(got, d_out)
    return rc, r.copy(), got, used


@pytest.mark.parametrize("mx", B.SWEEP_MAX)
def test_null_and_zero_budgets_change_nothing(clean, ora1, mx):
    e, cfg = clean
    rc0, res0, b0, u0 = e.fetch(PIDX1, CONS1, np.full(N1, mx))  # rmq_fetch
    rco, reso, bo, uo = ora1[0].fetch(PIDX1, CONS1, np.full(N1, mx))
    assert (rc0, u0) == (rco, uo) and np.array_equal(res0, reso) and np.array_equal(b0[:u0], bo[:uo]) and u0 > 0
    zeros = np.zeros(N1, np.uint32)
    for bud in (zeros, 0):
        rc1, res1, b1, u1 = e.fetch(PIDX1, CONS1, np.full(N1, mx), max_bytes=bud)
        assert (rc1, u1) == (rc0, u0) and np.array_equal(res1, res0) and np.array_equal(b1, b0)
    # rmq_fetch_bytes(max_bytes = NULL) itself, synchronous and asynchronous
    import ctypes as C
    for asyn in (False, True):
        req, res, out, used = _reqs(mx), np.zeros(N1, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8), C.c_uint64()
        args = (e.h, req.ctypes.data, None, N1, A.RMQ_MEM_HOST, out.ctypes.data, CAP, res.ctypes.data)
        if asyn:
            t = C.c_uint64()
            assert e.lib.rmq_fetch_bytes_async(*args, C.byref(t)) == A.RMQ_OK
            rc = e.lib.rmq_fetch_poll(e.h, t.value, 1, C.byref(used))
        else:
            rc = e.lib.rmq_fetch_bytes(*args, C.byref(used))
        assert (rc, used.value) == (rc0, u0) and np.array_equal(res, res0) and np.array_equal(out[:u0], b0[:u0])
        assert not out[u0:].any()
    # asynchronous host output with zero budgets
    out = np.full(CAP, 0xEE, np.uint8)
    tk = e.fetch_async(None, None, None, out=out, req=_reqs(mx), max_bytes=zeros)
    rca, resa, ua = e.fetch_poll(tk, wait=True)
    assert (rca, ua) == (rc0, u0) and np.array_equal(resa, res0) and np.array_equal(out[:ua], b0[:u0])
    assert (out[ua:] == 0xEE).all()
    # device output, ordinary and page-locked rows, synchronous and asynchronous
    d_out = e.device_alloc(CAP)
    try:
        for pinned in (False, True):
            req, res = e.fetch_rows(N1) if pinned else (np.zeros((N1, 4), np.uint32), np.zeros(N1, FETCH_RES_DTYPE))
            req[:] = _reqs(mx)
            for asyn in (False, True):
                rcd, resd, got, ud = _device_call(e, d_out, req, res, asyn, pinned, zeros)
                assert (rcd, ud) == (rc0, u0) and np.array_equal(resd, res0), (pinned, asyn)
                assert np.array_equal(got[:ud], b0[:u0]) and not got[ud:].any(), (pinned, asyn)
    finally:
        e.device_free(d_out)


@pytest.mark.parametrize("mx", B.SWEEP_MAX)
def test_sweep_on_state_1(clean, model1, mx):
    e, cfg = clean
    d_out = e.device_alloc(CAP)
    try:
        for b in B.SWEEP_BUDGETS:
            want = model1[(mx, b)]
            B.assert_equals_model(e.fetch(PIDX1, CONS1, np.full(N1, mx), max_bytes=b), want, (mx, b, "sync host"))
            out = np.zeros(CAP, np.uint8)
            tk = e.fetch_async(None, None, None, out=out, req=_reqs(mx), max_bytes=np.full(N1, b, np.uint64))
            rc, res, used = e.fetch_poll(tk, wait=True)
            B.assert_equals_model((rc, res, out, used), want, (mx, b, "async host"))
            req, res = e.fetch_rows(N1)
            req[:] = _reqs(mx)
            got = _device_call(e, d_out, req, res, b % 2 == 0, True, b)
            B.assert_equals_model(got, want, (mx, b, "device, page-locked rows"))
            e.host_release(req), e.host_release(res)
    finally:
        e.device_free(d_out)


def test_capacity_and_budgets_meet(clean, ora1):
    """One call with mixed budgets and an output smaller than needed: the trimmed bytes decide who fits."""
    e, cfg = clean
    ora = ora1[0]
    bud = np.array(B.SWEEP_BUDGETS + (0,), np.uint64)[np.arange(N1) % (len(B.SWEEP_BUDGETS) + 1)]
    full = B.model_fetch(ora, PIDX1, CONS1, 1024, bud)
    cap = (full[3] * 2 // 3) & ~15
    want = B.model_fetch(ora, PIDX1, CONS1, 1024, bud, out_cap=cap)
    _, res0, _, u0 = ora.fetch(PIDX1, CONS1, np.full(N1, 1024))
    assert want[0] == A.RMQ_ENOSPC and u0 > full[3] > cap
    nospc = (want[1]["status"] == A.RMQ_ENOSPC) & (want[1]["reserved"] == 0)
    served = (want[1]["status"] == A.RMQ_OK) & (want[1]["bytes"] > 0)
    assert nospc.any() and ((want[1]["status"] == A.RMQ_ENOSPC) & (want[1]["reserved"] > 0)).any()
    # a request that fits only because the requests before it were trimmed
    assert (served & (res0["out_pos"] + res0["bytes"] > cap)).any()
    B.assert_equals_model(e.fetch(PIDX1, CONS1, np.full(N1, 1024), out_cap=cap, max_bytes=bud), want)


def test_eoffset_row_keeps_its_answer(fresh_pair):
    e, ora, cfg = fresh_pair
    lo = ora.state(3)["log_start_offset"]
    for x in (e, ora):
        x.commit_consumer_offset(np.array([3], np.uint32), np.array([1], np.uint32), np.array([lo - 1], np.uint64))
    for b in (16, 512, 0xFFFFFFFF):
        want = B.model_fetch(ora, PIDX1, CONS1, 10, b)
        assert int(want[1]["status"][3 * B.NC1 + 1]) == A.RMQ_EOFFSET
        B.assert_equals_model(e.fetch(PIDX1, CONS1, np.full(N1, 10), max_bytes=b), want, b)


def test_cut_point_edges_on_state_3(oracle_mod):
    e, cfg = B.filled3(Engine)
    ora, _ = B.filled3(oracle_mod.OracleEngine)
    try:
        calls, big, _ = B.edge_calls3(ora, cfg)
        pidx, cons, mx = np.full(B.NC3, B.P3), np.arange(B.NC3), np.full(B.NC3, 0xFFFFFFFF)
        for k, bud in enumerate(calls):
            want = B.model_fetch(ora, pidx, cons, mx, bud)
            B.assert_equals_model(e.fetch(pidx, cons, mx, max_bytes=bud), want, k)
    finally:
        e.close()
        ora.close()


def test_grid_and_chunk_edges_on_state_4(oracle_mod):
    cfg = U.cfg4()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        U.fill4(e), U.fill4(ora)
        for n in B.N4:
            pidx, cons, mx, bud = B.reqs4(n)
            B.assert_equals_model(e.fetch(pidx, cons, mx, max_bytes=bud), B.model_fetch(ora, pidx, cons, mx, bud), n)


def _drain(e, ora, pidx, cons, replica):
    """Budget 512 with RMQ_FETCH_COMMIT until nothing is left, the model in step; the bytes each
    request got in all, and the sizes `reserved` named."""
    n = len(pidx)
    bud, got, named = np.full(n, 512, np.uint64), [b""] * n, []
    where = (lambda x, p: int(x.state(p)["high_watermark"]))
    for _ in range(64):
        before = [e.consumer_offsets(int(p)).copy() for p in pidx]
        want = B.model_fetch(ora, pidx, cons, 1024, bud, commit=True, replica=replica)
        rc, res, out, used = e.fetch(pidx, cons, np.full(n, 1024), commit=True, replica=replica, max_bytes=bud)
        B.assert_equals_model((rc, res, out, used), want)
        assert (res["bytes"] <= bud).all()
        for r in range(n):
            got[r] += out[int(res["out_pos"][r]):int(res["out_pos"][r]) + int(res["bytes"][r])].tobytes()
            if int(res["status"][r]) == A.RMQ_ENOSPC:  # nothing committed; the size to ask for
                assert int(res["reserved"][r]) > int(bud[r]) and int(res["count"][r]) == 0
                if not replica:
                    assert np.array_equal(e.consumer_offsets(int(pidx[r])), before[r]) or \
                        (pidx == pidx[r]).sum() > 1
                    assert int(e.consumer_offsets(int(pidx[r]))[int(cons[r])]) == int(res["start_offset"][r])
                named.append(int(res["reserved"][r]))
        bud = np.where(res["status"] == A.RMQ_ENOSPC, res["reserved"], 512).astype(np.uint64)
        if not res["count"].any() and not (res["status"] == A.RMQ_ENOSPC).any():
            return got, named
    raise AssertionError("the budgeted read never drained")


def test_budgeted_read_then_commit(fresh_pair, oracle_mod):
    e, ora, cfg = fresh_pair
    ref, _ = B.filled1(oracle_mod.OracleEngine)  # the whole unbudgeted read
    try:
        _, res0, b0, _ = ref.fetch(PIDX1, CONS1, np.full(N1, 1024))
        got, named = _drain(e, ora, PIDX1, CONS1, False)
        for r in range(N1):
            lo = int(res0["out_pos"][r])
            assert got[r] == b0[lo:lo + int(res0["bytes"][r])].tobytes(), r
        assert 1520 in named  # the 1,500-byte record: served by a retry with the budget it named
        for p in range(B.P1):
            assert np.array_equal(e.consumer_offsets(p), ora.consumer_offsets(p))
        # the same loop through the replica cursors
        pidx, cons = np.arange(B.P1), np.zeros(B.P1, np.uint32)
        starts = [x.state(p)["log_start_offset"] for x in (e,) for p in range(B.P1)]
        for x in (e, ora, ref):
            x.set_replica_cursor(pidx, starts)
        _, resr, br, _ = ref.fetch(pidx, cons, np.full(B.P1, 1024), replica=True)
        got, named = _drain(e, ora, pidx, cons, True)
        for r in range(B.P1):
            lo = int(resr["out_pos"][r])
            assert got[r] == br[lo:lo + int(resr["bytes"][r])].tobytes(), r
        assert 1520 in named
        # the position cache holds true pairs: an unbudgeted fetch from fresh mid offsets
        mid = []
        for p in PIDX1[::B.NC1]:
            st = ora.state(int(p))
            lo, hi = st["log_start_offset"], st["log_end_offset"]
            mid += [lo + (hi - lo) * (c + 1) // 6 for c in range(B.NC1)]
        for x in (e, ora):
            x.commit_consumer_offset(PIDX1.astype(np.uint32), CONS1.astype(np.uint32), np.array(mid, np.uint64))
        rc, res, out, used = e.fetch(PIDX1, CONS1, np.full(N1, 10))
        rco, reso, bo, uo = ora.fetch(PIDX1, CONS1, np.full(N1, 10))
        assert (rc, used) == (rco, uo) and np.array_equal(res, reso) and np.array_equal(out[:used], bo[:uo])
    finally:
        ref.close()


def test_verify_with_budgets(fresh_pair):
    e, ora, cfg = fresh_pair
    S = cfg.segment_bytes
    for b in (272, 512, 1520):
        plain = e.fetch(PIDX1, CONS1, np.full(N1, 10), max_bytes=b)
        B.assert_equals_model(e.fetch(PIDX1, CONS1, np.full(N1, 10), verify=True, max_bytes=b),
                              B.model_fetch(ora, PIDX1, CONS1, 10, b), b)
        assert np.array_equal(plain[1], B.model_fetch(ora, PIDX1, CONS1, 10, b)[1])
    # consumer 0 of partitions 3 and 2 stands at the log start: 12 records asked, cut after the fourth
    pidx, cons = np.array([3, 2]), np.array([0, 0])
    recs = [U.host_walk(e, cfg, 0, int(p))[2][:12] for p in pidx]
    size = lambda x: 16 + ((x[2] + 15) & ~15)  # noqa: E731
    bud = np.array([sum(size(x) for x in rr[:4]) + 8 for rr in recs], np.uint64)
    want = B.model_fetch(ora, pidx, cons, 12, bud, commit=True)
    assert list(want[5]) == [4, 4] and set(want[4]) == {"mid"}
    inside = next(x for x in recs[0][:4] if x[2] > 0)   # partition 3: a payload byte of the trimmed slice
    beyond = next(x for x in recs[1][4:] if x[2] > 0)   # partition 2: one of the slice before the cut only
    e.fault_flip_ring(0, 3, (inside[1] + 16) % S)
    e.fault_flip_ring(0, 2, (beyond[1] + 16) % S)
    before = e.consumer_offsets(3).copy()
    rc, res, out, used = e.fetch(pidx, cons, np.full(2, 12), commit=True, verify=True, max_bytes=bud)
    assert (rc, used) == (want[0], want[3])
    assert (int(res["status"][0]), int(res["count"][0])) == (A.RMQ_ECORRUPT, 0)
    assert all(int(res[f][0]) == int(want[1][f][0]) for f in ("start_offset", "out_pos", "bytes", "reserved"))
    assert np.array_equal(e.consumer_offsets(3), before)  # refused: nothing committed
    assert res[1] == want[1][1]  # the flip beyond the cut: served, and committed as the model's
    lo = int(res["out_pos"][1])
    assert np.array_equal(out[lo:lo + int(res["bytes"][1])], want[2][lo:lo + int(res["bytes"][1])])
    assert np.array_equal(e.consumer_offsets(2), ora.consumer_offsets(2))


def test_device_rows_with_a_device_budget_array(clean, model1):
    e, cfg = clean
    d_out, d_req, d_res, d_bud = e.device_alloc(CAP), e.device_alloc(16 * N1), e.device_alloc(32 * N1), e.device_alloc(4 * N1)
    try:
        e.h2d(d_req, _reqs(1024).view(np.uint8).reshape(-1))
        for b in B.SWEEP_BUDGETS:
            e.h2d(d_bud, np.full(N1, b, np.uint32).view(np.uint8))
            e.h2d(d_out, np.zeros(CAP, np.uint8))
            rc, _, used = e.fetch_device(None, None, None, d_out, CAP, d_rows=(N1, d_req, d_res, d_bud))
            res, got = np.zeros(N1, FETCH_RES_DTYPE), np.empty(CAP, np.uint8)
            e.d2h(res.view(np.uint8), d_res), e.d2h(got, d_out)
            B.assert_equals_model((rc, res, got, used), model1[(1024, b)], b)
    finally:
        for d in (d_out, d_req, d_res, d_bud):
            e.device_free(d)


@pytest.mark.parametrize("dma_in", ["0", "1"])
def test_rows_by_dma_with_budgets(monkeypatch, model1, dma_in):
    monkeypatch.setenv("RMQ_FETCH_DMA", "2")
    monkeypatch.setenv("RMQ_FETCH_DMA_IN", dma_in)
    e, cfg = B.filled1(Engine)
    try:
        for b in B.SWEEP_BUDGETS:
            want = model1[(1024, b)]
            B.assert_equals_model(e.fetch(PIDX1, CONS1, np.full(N1, 1024), max_bytes=b), want, (b, "sync"))
            req, res = e.fetch_rows(N1)
            req[:] = _reqs(1024)
            out = np.zeros(CAP, np.uint8)
            tk = e.fetch_async(None, None, None, out=out, req=req, res=res, pinned_rows=True, max_bytes=b)
            rc, r, used = e.fetch_poll(tk, wait=True)
            B.assert_equals_model((rc, r.copy(), out, used), want, (b, "async, page-locked rows"))
            e.host_release(req), e.host_release(res)
    finally:
        e.close()


def test_capacity_guarantee(clean, ora1):
    e, cfg = clean
    bud = np.array((16, 32, 256, 272, 512, 1520, 4096), np.uint64)[np.arange(N1) % 7]
    cap = int(bud.sum())
    want = B.model_fetch(ora1[0], PIDX1, CONS1, 1024, bud, out_cap=cap)
    rc, res, out, used = got = e.fetch(PIDX1, CONS1, np.full(N1, 1024), out_cap=cap, max_bytes=bud)
    assert rc == A.RMQ_OK and used <= cap
    assert not ((res["status"] == A.RMQ_ENOSPC) & (res["reserved"] == 0)).any()
    B.assert_equals_model(got, want)


def _segment_files(root):
    out = {}
    for path in sorted(glob.glob(os.path.join(root, "**", "*" + T.SEG_SUFFIX), recursive=True)):
        with open(path, "rb") as f:
            out[os.path.relpath(path, root)] = f.read()
    return out


def test_bounded_spill(tmp_path, oracle_mod):
    cfg = U.cfg3()
    parts = range(U.PARTS3)

    def filled():
        e = Engine(cfg)
        U.fill3(e)
        return e, np.array([e.state(p)["log_start_offset"] for p in parts], np.int64)

    with pytest.raises(ValueError):  # the oracle's fetch has no budgets
        with oracle_mod.OracleEngine(cfg) as o:
            T.DurableLog(o, str(tmp_path / "o"), parts, 0, spill_bytes=1 << 16)
    a, starts = filled()
    try:
        ref = T.DurableLog(a, str(tmp_path / "ref"), parts, 0, start=starts)
        moved = ref.spill()
        ref.close()
        want = _segment_files(str(tmp_path / "ref"))
        assert moved > 1000 and len(want) == U.PARTS3
    finally:
        a.close()
    b, _ = filled()
    try:
        log = T.DurableLog(b, str(tmp_path / "b64"), parts, 0, start=starts, spill_bytes=1 << 16)
        assert log.spill() == moved and log._buf.size <= 1 << 16
        log.close()
        assert _segment_files(str(tmp_path / "b64")) == want
        # the replica cursors end at the commits: nothing more to read
        _, res, _, _ = b.fetch(np.arange(U.PARTS3), np.zeros(U.PARTS3), np.full(U.PARTS3, 10), replica=True)
        assert [int(x) for x in res["start_offset"]] == [b.state(p)["high_watermark"] for p in parts]
        assert not res["count"].any()
    finally:
        b.close()
    # A buffer smaller than a record: the spill stops at the first record that cannot fit and names
    # its size. At 4 KiB that is the 8,224-byte record every retained log of state 3 starts with (the
    # sizes come from the oracle's log); at 16 KiB every record but the 16,400-byte one fits.
    with oracle_mod.OracleEngine(cfg) as o:
        U.fill3(o)
        sizes = B.sizes3(o, cfg)
    assert int(sizes[0]) == 8224 and int(sizes.max()) == 16400
    for cap, named in ((4096, 8224), (16384, 16400)):
        assert int(sizes[sizes > cap][0]) == named
        c, _ = filled()
        root = str(tmp_path / f"b{cap}")
        try:
            small = T.DurableLog(c, root, parts, 0, start=starts, spill_bytes=cap)
            with pytest.raises(EngineError) as ex:
                small.spill()
            assert ex.value.status == A.RMQ_ENOSPC and str(named) in str(ex.value), str(ex.value)
            assert small._buf.size <= cap
            small.close()
            part = _segment_files(root)
            assert all(want[k].startswith(v) for k, v in part.items()) and part != want
            assert (cap == 4096) == (not any(part.values()))  # (4 KiB: the very first record blocks)
            again = T.DurableLog(c, root, parts, 0, start=starts)  # a default spill completes the files
            assert again.spill() > 0
            again.close()
            assert _segment_files(root) == want
        finally:
            c.close()
