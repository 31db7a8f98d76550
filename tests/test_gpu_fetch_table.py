"""rmq_fetch_table on the GPU (FORMAT.md §7 "Record table"): every expected value is the model of
tests/fetch_table_util.py: the existing fetch models on the oracle for the rows and bytes, and
rmq_scan_records over the model's output for the table (tests/test_fetch_table_model.py shows that
each sweep here holds what it claims). For every call the rows, the output bytes of the served
ranges, bytes_used and the return code equal the model's, rec_row equals the model's whole, and
rec_pos equals the model's on every owned word and still holds its sentinel fill everywhere else."""
import ctypes as C

import numpy as np
import pytest

import fetch_at_util as FA
import fetch_budget_util as B
import fetch_fill_util as F
import fetch_table_util as T
import scrub_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import FETCH_RES_DTYPE, RESTORE_ITEM_DTYPE, Engine, table_records
from ripplemq_amd.state_machine import MessageBatchReadRequest, PartitionBroker, PartitionDirectory

pytestmark = pytest.mark.gpu

CAP = 1 << 18
GUARD = 8  # sentinel words past the table's capacity
N1 = B.P1 * B.NC1
PIDX1, CONS1 = B.all_reqs1()


@pytest.fixture(scope="module")
def ora1(oracle_mod):
    e, cfg = FA.filled1(oracle_mod.OracleEngine)  # (state 1, with room for the explicit requests' scratch ids)
    yield e, cfg
    e.close()


@pytest.fixture(scope="module")
def plain1(ora1):
    return {mx: T.plain1(ora1[0], mx) for mx in B.SWEEP_MAX}  # computed once, read by every test on state 1


@pytest.fixture(scope="module")
def clean():
    e, cfg = FA.filled1(Engine)
    yield e, cfg
    e.close()


@pytest.fixture()
def fresh_pair(oracle_mod):
    e, cfg = FA.filled1(Engine)
    o, _ = FA.filled1(oracle_mod.OracleEngine)
    yield e, o, cfg
    e.close()
    o.close()


def _need(want) -> int:
    return int(T.words_of(want[1]).sum())


def _reqs(pidx, cons, mx, flags=0):
    req = np.zeros((len(pidx), 4), np.uint32)
    req[:, 0], req[:, 1], req[:, 2], req[:, 3] = pidx, cons, mx, flags
    return req


def _check(got, want, cap, what):
    """got = (rc, rows, output, bytes_used, rec_row, rec_pos); the fetch against `want`, the table
    against its model at capacity cap (a table that overflows changes the return code alone)."""
    rc, res, out, used, row, pos = got
    rc_tab = T.expected(want, cap)[0]
    B.assert_equals_model((want[0] if rc == rc_tab else rc, res, out, used), want, what)
    T.assert_table(rc, row, pos, want, cap, what)


def _host(e, pidx, cons, mx, want, cap=None, out_cap=None, probe=False, **kw):
    """One call with ordinary rows, a host output and a host table of `cap` words (the model's need
    by default) inside sentinel-filled arrays."""
    cap = _need(want) if cap is None else cap
    row, pos = T.sentinel_arrays(len(pidx), cap + GUARD)
    got = e.fetch(pidx, cons, np.broadcast_to(mx, (len(pidx),)), out_cap=want[3] + 16 if out_cap is None else out_cap,
                  table=(row, None if probe else pos, cap), **kw)
    return got[:4] + (row, pos)


class DeviceCall:
    """Device output and device table for calls of up to n requests, sentinel-filled before each."""

    def __init__(self, e, n, out_cap, alloc):
        self.e, self.n, self.out_cap, self.alloc = e, n, out_cap, alloc
        self.d_out, self.d_row, self.d_pos = e.device_alloc(out_cap), e.device_alloc(8 * (n + 1)), e.device_alloc(8 * alloc)
        self.d_req, self.d_res, self.d_at = e.device_alloc(16 * n), e.device_alloc(32 * n), e.device_alloc(8 * n)

    def close(self):
        for d in (self.d_out, self.d_row, self.d_pos, self.d_req, self.d_res, self.d_at):
            self.e.device_free(d)

    def call(self, req, cap, offsets=None, rows="device", pinned=None, probe=False, **kw):
        e, n = self.e, len(req)
        assert n <= self.n and cap + GUARD <= self.alloc
        row, pos = T.sentinel_arrays(n, self.alloc)
        e.h2d(self.d_row, row.view(np.uint8)), e.h2d(self.d_pos, pos.view(np.uint8))
        e.h2d(self.d_out, np.zeros(self.out_cap, np.uint8))
        table = (self.d_row, 0 if probe else self.d_pos, cap)
        if rows == "device":
            e.h2d(self.d_req, np.ascontiguousarray(req).view(np.uint8).reshape(-1))
            if offsets is not None:
                e.h2d(self.d_at, np.ascontiguousarray(offsets, np.uint64).view(np.uint8))
            rc, _, used = e.fetch_device(None, None, None, self.d_out, self.out_cap, d_rows=(n, self.d_req, self.d_res),
                                         offsets=None if offsets is None else self.d_at, table=table, **kw)[:3]
            res = np.zeros(n, FETCH_RES_DTYPE)
            e.d2h(res.view(np.uint8), self.d_res)
        else:
            preq, pres = pinned
            preq[:n] = req
            rc, res, used = e.fetch_device(None, None, None, self.d_out, self.out_cap, req=preq[:n], res=pres[:n],
                                           pinned_rows=True, offsets=offsets, table=table, **kw)[:3]
            res = res.copy()
        out = np.empty(self.out_cap, np.uint8)
        e.d2h(out, self.d_out), e.d2h(row.view(np.uint8), self.d_row), e.d2h(pos.view(np.uint8), self.d_pos)
        return rc, res, out, used, row, pos


# ---- 1. state 1 with every kind of rows ----
@pytest.mark.parametrize("mx", B.SWEEP_MAX)
def test_state_1_ordinary_rows_host_output(clean, ora1, plain1, mx):
    e, cfg = clean
    _check(_host(e, PIDX1, CONS1, mx, plain1[mx]), plain1[mx], _need(plain1[mx]), (mx, "ordinary rows"))
    # state 1's committed offsets give no RMQ_EOFFSET row: fetch_at_util's explicit offsets do
    (pidx, cons, offs), want = T.explicit1(ora1[0], mx)
    assert A.RMQ_EOFFSET in want[1]["status"]
    _check(_host(e, pidx, cons, mx, want, offsets=offs), want, _need(want), (mx, "explicit offsets"))


@pytest.mark.parametrize("mx", B.SWEEP_MAX)
def test_state_1_pinned_rows_device_output(clean, ora1, plain1, mx):
    e, cfg = clean
    (pidx, cons, offs), want_at = T.explicit1(ora1[0], mx)
    d = DeviceCall(e, len(pidx), CAP, 4096)
    pinned = e.fetch_rows(len(pidx))
    try:
        want = plain1[mx]
        _check(d.call(_reqs(PIDX1, CONS1, mx), _need(want), rows="pinned", pinned=pinned), want, _need(want), (mx, "pinned"))
        _check(d.call(_reqs(pidx, cons, mx), _need(want_at), offsets=offs, rows="pinned", pinned=pinned), want_at,
               _need(want_at), (mx, "pinned, explicit offsets"))
    finally:
        d.close()
        e.host_release(pinned[0]), e.host_release(pinned[1])


@pytest.mark.parametrize("mx", B.SWEEP_MAX)
def test_state_1_device_rows_device_output_device_table(clean, ora1, plain1, mx):
    e, cfg = clean
    (pidx, cons, offs), want_at = T.explicit1(ora1[0], mx)
    d = DeviceCall(e, len(pidx), CAP, 4096)
    try:
        want = plain1[mx]
        _check(d.call(_reqs(PIDX1, CONS1, mx), _need(want)), want, _need(want), (mx, "device rows"))
        _check(d.call(_reqs(pidx, cons, mx), _need(want_at), offsets=offs), want_at, _need(want_at),
               (mx, "device rows, explicit offsets"))
    finally:
        d.close()


# ---- 2. state 3: the lane-count and window edges, big records first, inside and last ----
@pytest.fixture(scope="module")
def pair3(oracle_mod):
    cfg = U.cfg3()
    e, ora = Engine(cfg), oracle_mod.OracleEngine(cfg)
    U.fill3(e), U.fill3(ora)
    yield e, ora, cfg
    e.close()
    ora.close()


@pytest.mark.parametrize("variant", ["start", "big_first", "big_last"])
def test_state_3_counts_at_the_lane_and_window_edges(pair3, variant):
    e, ora, cfg = pair3
    (pidx, cons, mx, offs), want = T.model3(ora, cfg, variant)
    _check(_host(e, pidx, cons, mx, want, offsets=offs), want, _need(want), variant)
    if variant == "start":  # ... and written in place on the device
        d = DeviceCall(e, len(pidx), want[3] + 16, _need(want) + GUARD)
        try:
            _check(d.call(_reqs(pidx, cons, mx), _need(want), offsets=offs), want, _need(want), "device")
        finally:
            d.close()


# ---- 3. state 4: the scan's chunk edges, refused rows between owning ones ----
def test_state_4_request_counts_at_the_chunk_edges(oracle_mod):
    cfg = U.cfg4()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as ora:
        U.fill4(e), U.fill4(ora)
        for n in B.N4:
            (pidx, cons, mx), want = T.model4(ora, n)
            _check(_host(e, pidx, cons, mx, want), want, _need(want), n)
        d = DeviceCall(e, B.N4[-1], want[3] + 16, _need(want) + GUARD)
        try:
            for n in (257, 2500):
                (pidx, cons, mx), want = T.model4(ora, n)
                _check(d.call(_reqs(pidx, cons, mx), _need(want)), want, _need(want), (n, "device"))
        finally:
            d.close()


# ---- 4. budgets and fill with a table ----
def test_budgets_with_a_table(clean, ora1):
    e, cfg = clean
    ora = ora1[0]
    kinds = set()
    for b in B.SWEEP_BUDGETS:
        want = B.model_fetch(ora, PIDX1, CONS1, 1024, b)
        kinds |= {T.kind_of(want[1], r) for r in range(N1)}
        _check(_host(e, PIDX1, CONS1, 1024, want, max_bytes=b), want, _need(want), ("budget", b))
    assert {"owning", "enospc_budget"} <= kinds  # a cut row's words follow the cut; k* = 0 owns none
    # an output that is too small without RMQ_FETCH_FILL: the rows that do not fit own no words
    full = F.unbounded(ora, PIDX1, CONS1, 1024)
    cap = (full[3] // 2) & ~15
    small = B.model_fetch(ora, PIDX1, CONS1, 1024, 0, out_cap=cap)
    assert small[0] == A.RMQ_ENOSPC and "enospc_capacity" in {T.kind_of(small[1], r) for r in range(N1)}
    _check(_host(e, PIDX1, CONS1, 1024, small, out_cap=cap), small, _need(small), "output too small")


def test_fill_with_a_table(clean, ora1):
    e, cfg = clean
    ora = ora1[0]
    full = F.unbounded(ora, PIDX1, CONS1, 1024)
    d = DeviceCall(e, N1, CAP, 4096)
    kinds = set()
    try:
        for cap in T.fill_caps(full):
            want = F.model_fill(ora, PIDX1, CONS1, 1024, None, cap, full=full)
            kinds |= {T.kind_of(want[1], r) for r in range(N1)} | set(want[4])
            _check(_host(e, PIDX1, CONS1, 1024, want, out_cap=cap, fill=True), want, _need(want), ("fill", cap))
            d.out_cap = cap
            _check(d.call(_reqs(PIDX1, CONS1, 1024), _need(want), fill=True), want, _need(want), ("fill, device", cap))
            # a filling call returns RMQ_ENOSPC in one way only: the table does not fit
            got = _host(e, PIDX1, CONS1, 1024, want, cap=_need(want) - 1, out_cap=cap, fill=True)
            assert got[0] == A.RMQ_ENOSPC and got[3] <= cap and int(got[4][-1]) == _need(want)
            _check(got, want, _need(want) - 1, ("fill, table too small", cap))
    finally:
        d.close()
    assert {"owning", "pending", "cut_zero_pending"} <= kinds and kinds & {"cut_mid", "cut_boundary"}


def test_committing_calls_with_a_table_leave_the_oracles_consumer_table(fresh_pair):
    e, ora, cfg = fresh_pair
    want = B.model_fetch(ora, PIDX1, CONS1, 1024, 272, commit=True)
    _check(_host(e, PIDX1, CONS1, 1024, want, max_bytes=272, commit=True), want, _need(want), "budget, commit")
    assert np.array_equal(FA.tables(e), FA.tables(ora))
    full = F.unbounded(ora, PIDX1, CONS1, 10)
    cap = T.fill_caps(full)[0]
    want = F.model_fill(ora, PIDX1, CONS1, 10, None, cap, commit=True, full=full)
    _check(_host(e, PIDX1, CONS1, 10, want, out_cap=cap, fill=True, commit=True), want, _need(want), "fill, commit")
    assert np.array_equal(FA.tables(e), FA.tables(ora))


# ---- 5. table capacity ----
def test_table_capacity(clean, plain1):
    e, cfg = clean
    want = plain1[10]
    rec_row, _ = T.table_of(want[1], want[2])
    need = _need(want)
    owners = np.flatnonzero(T.words_of(want[1]))
    mid = int(owners[len(owners) // 2])
    inside = int(rec_row[mid]) + 1  # ends inside a middle row: that row and every later one stay unwritten
    d = DeviceCall(e, N1, CAP, need + 2 * GUARD)
    try:
        for cap, rc in ((need, A.RMQ_OK), (need - 1, A.RMQ_ENOSPC), (inside, A.RMQ_ENOSPC), (need + GUARD, A.RMQ_OK)):
            for got in (_host(e, PIDX1, CONS1, 10, want, cap=cap), d.call(_reqs(PIDX1, CONS1, 10), cap)):
                assert got[0] == rc
                _check(got, want, cap, ("capacity", cap))
        for got in (_host(e, PIDX1, CONS1, 10, want, cap=0, probe=True), d.call(_reqs(PIDX1, CONS1, 10), 0, probe=True)):
            assert got[0] == A.RMQ_ENOSPC and int(got[4][-1]) == need  # the size probe: rec_row alone
            _check(got, want, 0, "probe")
    finally:
        d.close()


def test_table_arguments(clean):
    e, cfg = clean
    req, res, used = _reqs(PIDX1, CONS1, 10), np.zeros(N1, FETCH_RES_DTYPE), C.c_uint64()
    out, row, pos = np.zeros(CAP, np.uint8), np.zeros(N1 + 1, np.uint64), np.zeros(64, np.uint64)

    def call(rec_row, rec_pos, rec_cap, n=N1):
        return e.lib.rmq_fetch_table(e.h, req.ctypes.data, None, None, n, A.RMQ_MEM_HOST, out.ctypes.data, CAP,
                                     res.ctypes.data, rec_row, rec_pos, rec_cap, C.byref(used))

    assert call(None, pos.ctypes.data, 64) == A.RMQ_EINVAL
    assert call(None, None, 64) == A.RMQ_EINVAL
    assert call(row.ctypes.data, None, 64) == A.RMQ_EINVAL
    assert call(None, None, 0) == A.RMQ_OK  # exactly rmq_fetch_at
    row[0] = 7
    assert call(row.ctypes.data, pos.ctypes.data, 64, n=0) == A.RMQ_OK and row[0] == 0  # rec_row has n + 1 words
    d = e.device_alloc(1024)
    try:  # device arrays are 8-byte aligned
        rc = e.lib.rmq_fetch_table(e.h, req.ctypes.data, None, None, N1, A.RMQ_MEM_DEVICE, C.c_void_p(d + 512), 256,
                                   res.ctypes.data, C.c_void_p(d + 4), C.c_void_p(d + 256), 8, C.byref(used))
        assert rc == A.RMQ_EINVAL
    finally:
        e.device_free(d)


def test_the_profiler_times_the_table_kernels(clean, plain1):
    e, cfg = clean
    want = plain1[10]
    e.profile(8)
    got = _host(e, PIDX1, CONS1, 10, want)
    calls, ms = e.profile_query(9)
    runs, spans = e.profile_query(4)[0], e.profile_query(3)[0]
    e.profile(0)
    assert (calls, runs, spans) == (1, 1, 0) and ms > 0  # once, without dispatch spans, as a budgeted call
    _check(got, want, _need(want), "profiled")


# ---- 6. verify ----
def _raw(e, req, out_cap, cap, alloc):
    n = len(req)
    res, out, used = np.zeros(n, FETCH_RES_DTYPE), np.zeros(out_cap, np.uint8), C.c_uint64()
    row, pos = T.sentinel_arrays(n, alloc)
    rc = e.lib.rmq_fetch_table(e.h, req.ctypes.data, None, None, n, A.RMQ_MEM_HOST, out.ctypes.data, out_cap,
                               res.ctypes.data, row.ctypes.data, pos.ctypes.data, cap, C.byref(used))
    return rc, res, out, int(used.value), row, pos


def test_a_refused_request_owns_no_words_and_its_unflagged_twin_does(fresh_pair):
    e, ora, cfg = fresh_pair
    S = cfg.segment_bytes
    pidx, cons = np.array([2, 3, 2, 4]), np.zeros(4, np.uint32)
    want = B.model_fetch(ora, pidx, cons, 12, 0)[:4]
    assert (want[1]["count"] == 12).all()
    rec = next(x for x in U.host_walk(e, cfg, 0, 2)[2][:12] if x[2] > 0)
    e.fault_flip_ring(0, 2, (rec[1] + 16) % S)  # a payload byte of the slice, on slot 0
    rc, res, out, used, row, pos = _raw(e, _reqs(pidx, cons, 12, [A.RMQ_FETCH_VERIFY, 0, 0, 0]), CAP, 64, 64)
    patched = want[1].copy()
    patched["status"][0], patched["count"][0] = A.RMQ_ECORRUPT, 0  # (start_offset, out_pos and bytes stay)
    assert (rc, used) == (A.RMQ_OK, want[3]) and np.array_equal(res, patched)
    for r in (1, 3):
        lo, hi = int(res["out_pos"][r]), int(res["out_pos"][r]) + int(res["bytes"][r])
        assert np.array_equal(out[lo:hi], want[2][lo:hi])
    # the later rows' rec_row move down by the refused row's 13 words; the twin (the same slice, the
    # same flipped payload byte, no flag) keeps the positions of the clean run
    T.assert_table(rc, row, pos, (rc, patched, want[2], used), 64, "verify")
    assert list(row) == [0, 0, 13, 26, 39]
    clean_row, clean_pos = T.table_of(want[1], want[2])
    assert np.array_equal(pos[13:26], clean_pos[0:13])


# ---- 7. a damaged length word under an unflagged request ----
def _damage_length(e, cfg, p, want_len):
    """Rewrites the length word of a record in the middle of partition p's retained log (slot 0) by
    byte flips; returns the record's index from the log start."""
    recs = U.host_walk(e, cfg, 0, p)[2]
    k = next(i for i in range(2, len(recs) - 2) if recs[i][2] >= 256)
    old = recs[k][2]
    new = want_len(old)
    for i in range(4):
        m = ((old >> (8 * i)) ^ (new >> (8 * i))) & 0xFF
        if m:
            e.fault_flip_ring(0, p, (recs[k][1] + 8 + i) % cfg.segment_bytes, m)
    return k, new


@pytest.mark.parametrize("name,want_len", [("smaller", lambda x: x & 0xFF), ("0xFFFFFFF0", lambda x: 0xFFFFFFF0)])
def test_a_damaged_length_word_keeps_the_table_bounded(fresh_pair, name, want_len):
    e, ora, cfg = fresh_pair
    pidx, cons = np.array([2, 3, 4]), np.zeros(3, np.uint32)  # consumer 0 stands at the log start
    want = B.model_fetch(ora, pidx, cons, 1024, 0)[:4]
    k, new = _damage_length(e, cfg, 3, want_len)
    assert int(want[1]["count"][1]) > k + 2
    need = _need(want)
    rc, res, out, used, row, pos = _raw(e, _reqs(pidx, cons, 1024), CAP, need, need + GUARD)
    # the slices run from the log start to the high watermark: no length word places them
    assert (rc, used) == (want[0], want[3]) and np.array_equal(res, want[1])
    clean_row, clean_pos = T.table_of(want[1], want[2])
    assert np.array_equal(row, clean_row)
    a, b, nb = int(row[1]), int(row[2]), int(res["bytes"][1])
    assert np.array_equal(pos[:a], clean_pos[:a]) and np.array_equal(pos[b:need], clean_pos[b:need])  # the rows around it
    assert (pos[need:] == T.SENT).all()
    words = pos[a:b]
    lo = int(res["out_pos"][1])
    run = out[lo:lo + nb]
    assert int.from_bytes(run[int(clean_pos[a + k]) + 8:][:4].tobytes(), "little") == new  # the damage is in the run
    assert words[0] == 0 and words[-1] == nb and not (words % 16).any() and (words <= nb).all()
    assert np.array_equal(words[:k + 1], clean_pos[a:a + k + 1])  # true starts up to the damaged record
    assert np.array_equal(words, T.reference_walk(run, int(res["count"][1])))
    assert not np.array_equal(words, clean_pos[a:b])
    if name == "0xFFFFFFF0":
        assert (words[k + 1:] == nb).all()


# ---- 8. restore from a fetched table, no host walk ----
def test_restore_from_a_fetched_table(pair3):
    e, ora, cfg = pair3
    parts = np.arange(U.PARTS3)
    st = [e.state(int(p)) for p in parts]
    offs = np.array([s["log_start_offset"] for s in st], np.uint64)
    cons, mx = np.zeros(len(parts), np.uint32), np.full(len(parts), 0xFFFFFFFF, np.uint32)
    want = FA.model_fetch_at(ora, parts, cons, mx, offs, replica=True)
    rc, res, buf, used, rec_row, rec_pos = e.fetch(parts, cons, mx, replica=True, offsets=offs, table=True)
    B.assert_equals_model((rc, res, buf, used), want, "replica fetch")
    T.assert_table(rc, rec_row, rec_pos[:int(rec_row[-1])], want, int(rec_row[-1]), "replica fetch")
    items = np.zeros(len(parts), RESTORE_ITEM_DTYPE)
    for r, p in enumerate(parts):
        items[r] = (p, 0, res["start_offset"][r], st[r]["log_start_pos"], res["count"][r], res["bytes"][r],
                    res["out_pos"][r], rec_row[r], int(res["start_offset"][r]) + int(res["count"][r]))
    with Engine(cfg) as fresh:
        rows = fresh.restore(items, buf, rec_pos)
        assert fresh.last_restore_rc == A.RMQ_OK and (rows["status"] == A.RMQ_OK).all()
        assert np.array_equal(rows["records"], res["count"]) and np.array_equal(rows["bytes"], res["bytes"])
        scrub = fresh.scrub()
        assert (scrub["status"] == A.RMQ_OK).all() and (scrub["bad_offset"] == A.RMQ_OFFSET_NONE).all()
        assert np.array_equal(scrub["records_ok"], res["count"].astype(np.uint64) * scrub["replicas"])
        rc2, res2, buf2, used2 = fresh.fetch(parts, cons, mx, replica=True, offsets=offs)
        assert (rc2, used2) == (rc, used) and np.array_equal(res2, res) and np.array_equal(buf2[:used], buf[:used])


# ---- 9. the broker's batch read split by the table ----
def test_batch_read_with_a_record_table_answers_the_same(clean):
    e, cfg = clean
    d = PartitionDirectory({"t": B.P1}, max_consumers=cfg.max_consumers)
    for c in range(B.NC1):
        assert d.consumer(f"c{c}") == c
    plain = PartitionBroker(d, engine=e, messages_as_str=False)
    tabled = PartitionBroker(d, engine=e, messages_as_str=False, record_table=True)
    for mx in B.SWEEP_MAX:
        reqs = [MessageBatchReadRequest(f"c{c}", mx, "t", int(p)) for p, c in zip(PIDX1, CONS1)]
        a, b = plain.process_batch_read(reqs), tabled.process_batch_read(reqs)
        assert len(a) == len(b) == N1
        assert [(x.getMessages(), x.getOffset(), x.isSuccess()) for x in a] == \
               [(x.getMessages(), x.getOffset(), x.isSuccess()) for x in b]
        assert sum(len(x.getMessages()) for x in a) > N1 // 2


# ---- 10. asynchronous tickets ----
def test_async_table_tickets_around_a_held_back_one(clean, plain1):
    """Four table tickets in flight with an ordinary, held-back ticket between them: each completes
    with its own rows, bytes and table."""
    e, cfg = clean
    mxs = (1, 10, None, 1024, 10)  # (None: the ordinary ticket)
    outs = [np.zeros(CAP, np.uint8) for _ in mxs]
    tabs, tks = [], []
    for k, mx in enumerate(mxs):
        if mx is None:
            tabs.append(None)
            tks.append(e.fetch_async(None, None, None, out=outs[k], req=_reqs(PIDX1, CONS1, 10)))
            continue
        need = _need(plain1[mx])
        tabs.append(T.sentinel_arrays(N1, need + GUARD) + (need,))
        tks.append(e.fetch_async(None, None, None, out=outs[k], req=_reqs(PIDX1, CONS1, mx), table=tabs[k]))
    for k, mx in enumerate(mxs):
        got = e.fetch_poll(tks[k], wait=True)
        if mx is None:
            rc, res, used = got
            B.assert_equals_model((rc, res, outs[k], used), plain1[10], "ordinary ticket")
            continue
        rc, res, used, row, pos = got
        assert row is tabs[k][0] and pos is tabs[k][1]
        _check((rc, res, outs[k], used, row, pos), plain1[mx], tabs[k][2], ("ticket", k))
        assert table_records(outs[k], res, row, pos)[0] is not None
