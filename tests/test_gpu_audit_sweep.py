"""A differential sweep of the two audit kernels (FORMAT.md §10): rmq_scrub and RMQ_FETCH_VERIFY over
record lengths at every piece-count edge (state 3), every byte of one log flipped (state 1), 2500
partitions (state 4), the grid-stride loops (RMQ_AUDIT_WGS and a ticket larger than the grid) and
the position cache after a refusal. Every expected value comes from the host walk
(tests/scrub_util.py), the CPU oracle or the call without the flag, never from the kernel under
test; tests/test_audit_states.py checks the states and the flip list on the CPU."""
import time

import numpy as np
import pytest

import scrub_util as U
from parity import compare_state, ring_window, run_ops
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine
from ripplemq_amd.workload import Batch
from test_gpu_scrub import KINDS, _pick

pytestmark = pytest.mark.gpu

V, CM = A.RMQ_FETCH_VERIFY, A.RMQ_FETCH_COMMIT
CRC, CHAIN = A.RMQ_SCRUB_BAD_CRC, A.RMQ_SCRUB_BAD_CHAIN
OK, ECORRUPT, ENOSPC = A.RMQ_OK, A.RMQ_ECORRUPT, A.RMQ_ENOSPC
FILL = 0xEE


def _reqs(pidx, cons, mx, flags=0):
    req = np.zeros((len(pidx), 4), np.uint32)
    req[:, 0], req[:, 1], req[:, 2], req[:, 3] = pidx, cons, mx, flags
    return req


def _call(e, req, cap):
    """One rmq_fetch_async + poll of the rows `req` into a host buffer: (rc, rows copy, bytes, used)."""
    out = np.full(cap, FILL, np.uint8)
    tk = e.fetch_async(None, None, None, out=out, req=req.copy())
    rc, res, used = e.fetch_poll(tk, wait=True)
    return rc, res.copy(), out, used


def _commit(engines, pidx, cons, offs):
    for e in engines:
        rc, st = e.commit_consumer_offset(np.array(pidx, np.uint32), np.array(cons, np.uint32), np.array(offs, np.uint64))
        assert rc == 0 and not st.any()


def _refused(row, clean):
    """`row` is the refusal of the request served as `clean`: RMQ_ECORRUPT, count 0, its place kept."""
    return (int(row["status"]), int(row["count"]), int(row["start_offset"]), int(row["out_pos"]), int(row["bytes"])) == \
        (ECORRUPT, 0, int(clean["start_offset"]), int(clean["out_pos"]), int(clean["bytes"]))


def _scrub_row(r):
    return int(r["status"]), int(r["bad_offset"]), int(r["bad_replica"])


# ---------------------------------------------------------------------------------------------
# state 3: length edges
# ---------------------------------------------------------------------------------------------
NC3 = 256


@pytest.fixture(scope="module")
def state3(oracle_mod):
    """State 3 on the engine and on the oracle, appended through parity.run_ops with whole rings
    compared after every batch (the apply stage's CRC at every listed length, bit for bit); then
    consumer c of every partition stands at log start + c."""
    cfg = U.cfg3()
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as o:
        log = run_ops(e, o, cfg, [("append", Batch(*U.batch3(b))) for b in range(U.BATCHES3)], full_rings=True)
        assert all(st["appended"] == U.PARTS3 * len(U.LENS3) for _, st in log)
        recs = [U.host_walk(e, cfg, 0, p)[2] for p in range(U.PARTS3)]
        for p in range(U.PARTS3):
            assert len(recs[p]) >= NC3
            _commit((e, o), [p] * NC3, range(NC3), [recs[p][0][0] + c for c in range(NC3)])
        yield e, o, cfg, recs


def test_length_edges_append_parity(state3):
    e, o, cfg, recs = state3
    compare_state(e, o, cfg, full_rings=True)
    for p in range(U.PARTS3):
        st = e.state(p)
        assert st["log_end_offset"] == U.BATCHES3 * len(U.LENS3) and st["log_start_offset"] > 0
        assert {ln for _, _, ln in recs[p]} == set(U.LENS3)


def test_length_edges_scrub_clean(state3):
    e, o, cfg, recs = state3
    rows = e.scrub()
    assert e.last_scrub_rc == OK
    U.assert_clean(rows, e, cfg)
    for p in range(U.PARTS3):
        for r in range(cfg.replication_factor):
            k, bad, _, st = U.host_walk(e, cfg, r, p)
            assert bad == U.NONE and k == st["log_end_offset"] - st["log_start_offset"], (p, r)


def test_length_edges_whole_log_slices(state3):
    e, o, cfg, recs = state3
    pidx, cons, mx = np.arange(U.PARTS3), np.zeros(U.PARTS3), np.full(U.PARTS3, 1024)
    rc0, res0, b0, u0 = e.fetch(pidx, cons, mx)
    rc1, res1, b1, u1 = e.fetch(pidx, cons, mx, verify=True)
    rco, reso, bo, uo = o.fetch(pidx, cons, mx)
    assert rc0 == rc1 == rco == OK and u0 == u1 == uo == int(res0["bytes"].sum())
    assert (res0["status"] == 0).all() and [int(x) for x in res0["count"]] == [len(r) for r in recs]
    assert int(res0["count"].min()) > 128  # more than two passes of 64 records
    assert np.array_equal(res1, res0) and np.array_equal(b1, b0)
    assert np.array_equal(reso, res0) and np.array_equal(bo[:uo], b0[:u0])


@pytest.mark.parametrize("mx", [1, 3])
def test_length_edges_one_record_slices(state3, mx):
    e, o, cfg, recs = state3
    for p in range(U.PARTS3):  # the 256 consumers stand on every large length
        assert set(U.BIG3) <= {ln for _, _, ln in recs[p][:NC3]}
    pidx, cons = np.repeat(np.arange(U.PARTS3), NC3), np.tile(np.arange(NC3), U.PARTS3)
    cap = 1 << 23
    rc0, res0, out0, u0 = _call(e, _reqs(pidx, cons, mx), cap)
    rc1, res1, out1, u1 = _call(e, _reqs(pidx, cons, mx, V), cap)
    rco, reso, bo, uo = o.fetch(pidx, cons, np.full(len(pidx), mx), out_cap=cap)
    assert rc0 == rc1 == rco == OK and u0 == u1 == uo <= cap
    assert (res0["status"] == 0).all() and (res0["count"] == mx).all()
    assert np.array_equal(res1, res0) and np.array_equal(out1, out0)
    assert np.array_equal(reso, res0) and np.array_equal(bo[:uo], out0[:u0]) and (out0[u0:] == FILL).all()


def _edge_flips(recs):
    """[(label, record index, byte of the record)] on slot 0 of one partition of state 3."""
    out = []
    idx = {ln: next(i for i, x in enumerate(recs) if x[2] == ln and 0 < i < NC3 - 1) for ln in (1025, 4097, 12289, 16384, 4096)}
    for ln in (1025, 4097, 12289, 16384):
        i = idx[ln]
        pieces = (ln + 15) // 16
        for k in (0, 63, 64, 255, 256):
            if k < pieces:
                out.append((f"{ln}B piece {k}", i, 16 + 16 * k + min(5, ln - 16 * k - 1)))
        out.append((f"{ln}B last payload byte", i, 16 + ln - 1))
        if ln % 16:
            out.append((f"{ln}B first padding byte", i, 16 + ln))
    out.append(("4096B stored crc", idx[4096], 13))
    for label, i in (("record 0", 0), ("record >= 64", next(i for i in range(64, 128) if recs[i][2])),
                     ("record >= 128", next(i for i in range(128, 192) if recs[i][2])), ("last record", len(recs) - 1)):
        out.append((label, i, 16 + recs[i][2] // 2 if recs[i][2] else 12))  # (an empty record: a crc byte)
    return out


def test_length_edges_targeted_flips(state3):
    e, o, cfg, recs_all = state3
    S, p = cfg.segment_bytes, 1
    recs = recs_all[p]
    flips = _edge_flips(recs)
    assert len(flips) >= 30 and len(recs) > 129
    whole = _reqs([p], [0], 1024, V)
    rcw, resw, _, uw = _call(e, whole, 1 << 20)
    assert rcw == OK and int(resw["count"][0]) == len(recs) and int(resw["status"][0]) == 0
    clean_rows = e.scrub()
    U.assert_clean(clean_rows, e, cfg)
    for label, i, d in flips:
        rec = recs[i]
        ring_off = (rec[1] + d) % S
        near = [c for c in (i - 1, i, i + 1) if 0 <= c < NC3 and c < len(recs)]  # the record's consumer and its neighbours'
        one = _reqs([p] * len(near), near, 1, V)
        rcc, resc, outc, uc = _call(e, one, 1 << 16) if near else (OK, None, None, 0)
        e.fault_flip_ring(0, p, ring_off)
        try:
            rows = e.scrub()
            bad = U.host_walk(e, cfg, 0, p)[1]
            rc1, res1, _, u1 = _call(e, whole, 1 << 20)
            rc2, res2, out2, u2 = _call(e, one, 1 << 16) if near else (OK, None, None, 0)
        finally:
            e.fault_flip_ring(0, p, ring_off)
        assert bad == rec[0], (label, bad, rec)
        assert _scrub_row(rows[p]) == (ECORRUPT, bad, 0) and int(rows[p]["bad_kind"]) == CRC, (label, rows[p], bad)
        others = np.arange(U.PARTS3) != p
        assert np.array_equal(rows[others], clean_rows[others]), label
        assert rc1 == OK and u1 == uw and _refused(res1[0], resw[0]), (label, res1, resw)
        if near:
            assert rcc == rc2 == OK and u2 == uc, label
            for k, c in enumerate(near):
                if c == i:
                    assert _refused(res2[k], resc[k]), (label, res2[k], resc[k])
                else:
                    assert np.array_equal(res2[k:k + 1], resc[k:k + 1]), (label, c, res2[k], resc[k])
                    lo, hi = int(resc["out_pos"][k]), int(resc["out_pos"][k]) + int(resc["bytes"][k])
                    assert np.array_equal(out2[lo:hi], outc[lo:hi]), (label, c)
        after = e.scrub()  # flipped back: clean again
        assert e.last_scrub_rc == OK and np.array_equal(after, clean_rows), label
    rc1, res1, _, _ = _call(e, whole, 1 << 20)
    assert rc1 == OK and np.array_equal(res1, resw)


# ---------------------------------------------------------------------------------------------
# state 1: every byte of one log
# ---------------------------------------------------------------------------------------------
def _consumers1(engines, cfg):
    """Consumers at the log start, inside, near the end and at the end of every partition (as
    tests/test_gpu_fetch_verify.py places them)."""
    e = engines[0]
    pidx, cons, offs = [], [], []
    for p in range(cfg.num_partitions):
        st = e.state(p)
        lo, hi = st["log_start_offset"], st["log_end_offset"]
        for c, o in enumerate((lo, lo + (hi - lo) // 3, max(lo, hi - 2), hi)):
            pidx.append(p), cons.append(c), offs.append(o)
    _commit(engines, pidx, cons, offs)


def _state1(oracle_mod=None):
    cfg = U.cfg1()
    e = Engine(cfg)
    U.fill1(e)
    engines = [e]
    if oracle_mod is not None:
        o = oracle_mod.OracleEngine(cfg)
        U.fill1(o)
        engines.append(o)
    _consumers1(engines, cfg)
    return (*engines, cfg)


@pytest.fixture()
def fresh1():
    e, cfg = _state1()
    yield e, cfg
    e.close()


def _sweep(e, cfg, slot):
    p = U.SWEEP_P
    st = e.state(p)
    win = ring_window(e, cfg, slot, p, st)
    _, bad, recs, _ = U.walk_window(win, st)
    assert bad == U.NONE and len(recs) > len(U.LENS1) and 3000 < win.size <= cfg.segment_bytes
    flips = U.sweep_positions(recs)
    if U.SWEEP_STRIDE is None:
        assert [w for w, _, _ in flips] == list(range(win.size))
    return st, win, recs, flips


def test_every_byte_scrub(fresh1):
    """Every byte of partition 3's retained log flipped on slot 2, one scrub each: the row names the
    host walk's offset and the slot, the kind by the byte's place in the record, and the other
    rows stay clean with exact totals. Measured on an MI355X: 66 to 71 us per scrub call of this
    state, the 3,376 flips (flip, scrub, flip back, host walk) in 0.45 to 0.52 s, so no position is
    left out (scrub_util.SWEEP_STRIDE stays None)."""
    e, cfg = fresh1
    S, p, slot = cfg.segment_bytes, U.SWEEP_P, U.SWEEP_SCRUB_SLOT
    st, win, recs, flips = _sweep(e, cfg, slot)
    clean_rows = e.scrub()
    U.assert_clean(clean_rows, e, cfg)
    t0 = time.perf_counter()
    for _ in range(20):
        e.scrub()
    print(f"scrub of state 1: {(time.perf_counter() - t0) / 20 * 1e6:.0f} us per call")
    others = np.arange(cfg.num_partitions) != p
    wrong = []
    t0 = time.perf_counter()
    for w, i, d in flips:
        ring_off = (st["log_start_pos"] + w) % S
        win[w] ^= U.SWEEP_MASK
        bad = U.walk_window(win, st)[1]
        win[w] ^= U.SWEEP_MASK
        e.fault_flip_ring(slot, p, ring_off, U.SWEEP_MASK)
        try:
            rows = e.scrub()
            rc = e.last_scrub_rc
        finally:
            e.fault_flip_ring(slot, p, ring_off, U.SWEEP_MASK)
        kinds = {CHAIN} if d < 8 else {CRC, CHAIN} if d < 12 else {CRC}
        r = rows[p]
        if not (bad == recs[i][0] and rc == ECORRUPT and _scrub_row(r) == (ECORRUPT, bad, slot) and int(r["bad_kind"]) in kinds
                and int(r["replicas"]) == 3 and np.array_equal(rows[others], clean_rows[others])):
            wrong.append((w, i, d, bad, r))
    print(f"scrub sweep: {len(flips)} flips in {time.perf_counter() - t0:.2f} s")
    assert not wrong, (len(wrong), wrong[:8])
    assert np.array_equal(e.scrub(), clean_rows) and e.last_scrub_rc == OK  # every flip undone


def test_every_byte_fetch_verify(fresh1):
    """Every byte of partition 3's retained log flipped on slot 0, one call each of two unflagged
    requests and the flagged, committing whole-log request, into a 64 KiB device output: the
    flagged request is never served and never commits, and nothing else in the call changes.
    Measured on an MI355X: 76 to 83 us per call with the output's fill and read-back, the 3,376
    flips in 0.52 to 0.60 s."""
    e, cfg = fresh1
    S, p, cap = cfg.segment_bytes, U.SWEEP_P, 1 << 16
    st, win, recs, flips = _sweep(e, cfg, 0)
    req = _reqs((1, 2, p), (0, 0, 0), (4, 4, 1024), (0, 0, V | CM))
    probe = _reqs((1, 2, p), (0, 0, 0), (4, 4, 1024), (0, 0, V))
    fill = np.full(cap, FILL, np.uint8)
    got = np.empty(cap, np.uint8)
    d_out = e.device_alloc(cap)
    try:
        def run(rq):
            e.h2d(d_out, fill)
            rc, res, used = e.fetch_device(None, None, None, d_out, cap, req=rq.copy())
            e.d2h(got, d_out)
            return rc, res.copy(), used
        rc0, res0, u0 = run(probe)  # (the clean call commits nothing: the flips below start from the same offset)
        got0 = got.copy()
        assert rc0 == OK and (res0["status"] == 0).all() and [int(x) for x in res0["count"]] == [4, 4, len(recs)]
        lo, nb = int(res0["out_pos"][2]), int(res0["bytes"][2])
        assert nb == win.size and lo + nb == u0 and np.array_equal(got0[lo:u0], win) and (got0[u0:] == FILL).all()
        offs0 = e.consumer_offsets(p).copy()
        t0 = time.perf_counter()
        for _ in range(20):
            run(probe)
        print(f"flagged fetch of state 1 (with the output's fill and read-back): {(time.perf_counter() - t0) / 20 * 1e6:.0f} us per call")
        wrong = []
        t0 = time.perf_counter()
        for w, i, d in flips:
            ring_off = (st["log_start_pos"] + w) % S
            e.fault_flip_ring(0, p, ring_off, U.SWEEP_MASK)
            try:
                rc, res, used = run(req)
            finally:
                e.fault_flip_ring(0, p, ring_off, U.SWEEP_MASK)
            r = res[2]
            ok = np.array_equal(res[:2], res0[:2]) and np.array_equal(got[:lo], got0[:lo])
            ok = ok and np.array_equal(e.consumer_offsets(p), offs0)
            if 8 <= d < 12:  # a length word: the resolve walks it, so bytes may differ; never served
                hi = min(int(r["out_pos"]) + int(r["bytes"]), cap)
                ok = ok and int(r["count"]) == 0 and int(r["status"]) in (ECORRUPT, ENOSPC) and int(r["out_pos"]) == lo
                ok = ok and int(r["start_offset"]) == int(res0["start_offset"][2]) and (got[max(hi, lo):] == FILL).all()
            else:  # the refused bytes lie in a device output as they are in the ring
                win[w] ^= U.SWEEP_MASK
                ok = ok and rc == OK and used == u0 and _refused(r, res0[2]) and np.array_equal(got[lo:u0], win)
                win[w] ^= U.SWEEP_MASK
                ok = ok and (got[u0:] == FILL).all()
            if not ok:
                wrong.append((w, i, d, rc, used, r))
        print(f"fetch sweep: {len(flips)} flips in {time.perf_counter() - t0:.2f} s")
        assert not wrong, (len(wrong), wrong[:8])
        rc1, res1, u1 = run(req)  # every flip undone: served, and now it commits
        assert (rc1, u1) == (rc0, u0) and np.array_equal(res1, res0) and np.array_equal(got, got0)
        assert int(e.consumer_offsets(p)[0]) == int(offs0[0]) + len(recs)
    finally:
        e.device_free(d_out)


def _padding_case(e, cfg, crc32c, p, recs, ln, whole_count):
    """Non-zero padding under which the record's CRC over its padded pieces still matches
    (scrub_util.crc_consistent_padding), on slot 0: only the zero-padding rule refuses it."""
    S = cfg.segment_bytes
    rec = next(x for x in recs if x[2] == ln)
    st = e.state(p)
    win = ring_window(e, cfg, 0, p, st)
    a = rec[1] - st["log_start_pos"] + 16
    pad = -ln % 16
    bad = U.crc_consistent_padding(win[a:a + ln].tobytes(), pad, crc32c)
    whole = _reqs([p], [0], 1024, V)
    rc0, res0, _, u0 = _call(e, whole, 1 << 20)
    assert rc0 == OK and (int(res0["status"][0]), int(res0["count"][0])) == (0, whole_count)
    clean_rows = e.scrub()
    flips = [((rec[1] + 16 + ln + k) % S, b) for k, b in enumerate(bad) if b]
    for ring_off, b in flips:
        e.fault_flip_ring(0, p, ring_off, b)
    try:
        rows = e.scrub()
        host = U.host_walk(e, cfg, 0, p)[1]
        rc1, res1, _, u1 = _call(e, whole, 1 << 20)
    finally:
        for ring_off, b in flips:
            e.fault_flip_ring(0, p, ring_off, b)
    assert host == rec[0], (ln, host, rec)
    assert _scrub_row(rows[p]) == (ECORRUPT, rec[0], 0) and int(rows[p]["bad_kind"]) == CRC, (ln, rows[p])
    assert (rc1, u1) == (rc0, u0) and _refused(res1[0], res0[0]), (ln, res1, res0)
    assert np.array_equal(e.scrub(), clean_rows) and e.last_scrub_rc == OK
    rc1, res1, _, _ = _call(e, whole, 1 << 20)
    assert np.array_equal(res1, res0)


def test_crc_consistent_padding_lane_path(fresh1, oracle_mod):
    e, cfg = fresh1
    recs = U.host_walk(e, cfg, 0, U.SWEEP_P)[2]
    for ln in (17, 241, 600):  # records of at most 64 pieces: a lane each
        _padding_case(e, cfg, oracle_mod.crc32c, U.SWEEP_P, recs, ln, len(recs))


def test_crc_consistent_padding_wave_path(state3, oracle_mod):
    e, o, cfg, recs = state3
    for ln in (1025, 4097, 12289):  # over 64 pieces: the whole wave, the last piece read again
        _padding_case(e, cfg, oracle_mod.crc32c, 2, recs[2], ln, len(recs[2]))


# ---------------------------------------------------------------------------------------------
# state 4: many partitions
# ---------------------------------------------------------------------------------------------
SUBRANGES = ((1000, 1100), (1, 1024), (1024, 1476), (2499, 1))


def _state4():
    cfg = U.cfg4()
    e = Engine(cfg)
    U.fill4(e)
    return e, cfg


@pytest.fixture(scope="module")
def state4():
    e, cfg = _state4()
    yield e, cfg
    e.close()


def _marked_flips(e, cfg, slots, index=None):
    """A stored-CRC byte of one record of each marked partition: [(partition, slot, ring offset,
    record)], the middle record or record `index(k)`."""
    out = []
    for k, p in enumerate(U.MARKED4):
        recs = U.host_walk(e, cfg, slots[k % len(slots)], p)[2]
        assert len(recs) >= 5
        rec = recs[len(recs) // 2 if index is None else index(k)]
        out.append((p, slots[k % len(slots)], (rec[1] + 12) % cfg.segment_bytes, rec))
    return out


def _flip_all(e, flips):
    for p, slot, ring_off, _ in flips:
        e.fault_flip_ring(slot, p, ring_off)


def _assert_marked_rows(rows, first, flips, clean_rows):
    """Rows of scrub(first, len(rows)) under `flips`: the flipped partitions in range are named at
    their host-walk offsets and slots, every other row is the clean one."""
    hit = np.zeros(len(rows), bool)
    for p, slot, _, rec in flips:
        if first <= p < first + len(rows):
            hit[p - first] = True
            r = rows[p - first]
            assert _scrub_row(r) == (ECORRUPT, rec[0], slot) and int(r["bad_kind"]) == CRC and int(r["replicas"]) == 2, (p, r, rec)
    assert np.array_equal(rows[~hit], clean_rows[first:first + len(rows)][~hit])
    return int(hit.sum())


def test_many_partitions_scrub(state4):
    e, cfg = state4
    states = e.states()
    assert U.scrub_tasks(states, cfg) > 2 * 64 * 64
    rows = e.scrub()
    assert e.last_scrub_rc == OK and len(rows) == U.P4
    U.assert_clean_bulk(rows, states, 2)  # replicas == 2 on empty partitions too
    assert int((rows["records_ok"] == 0).sum()) >= 800
    for first, n in SUBRANGES:
        assert np.array_equal(e.scrub(first, n), rows[first:first + n]), (first, n)
    flips = _marked_flips(e, cfg, (0, 1))
    _flip_all(e, flips)
    try:
        for p, slot, _, rec in flips:  # the host walk stops at each flipped record
            assert U.host_walk(e, cfg, slot, p)[1] == rec[0], p
        bad_rows = e.scrub()
        rc = e.last_scrub_rc
        sub = e.scrub(1000, 1100)
    finally:
        _flip_all(e, flips)
    assert rc == ECORRUPT
    assert _assert_marked_rows(bad_rows, 0, flips, rows) == 8
    assert _assert_marked_rows(sub, 1000, flips, rows) == 4  # 1023, 1024, 2047 and 2048
    assert np.array_equal(e.scrub(), rows) and e.last_scrub_rc == OK


def _fetch4(e, flags):
    pidx = np.arange(U.P4)
    return _call(e, _reqs(pidx, np.zeros(U.P4), 4, flags), 1 << 21)


def _assert_fetch4(e, flips, clean):
    """The 2500-row flagged ticket under `flips` on slot 0: the rows whose first four records hold
    a flipped one are refused, every other row and its bytes are the clean call's."""
    rc0, res0, out0, u0 = clean
    _flip_all(e, flips)
    try:
        rc1, res1, out1, u1 = _fetch4(e, V)
    finally:
        _flip_all(e, flips)
    assert (rc1, u1) == (rc0, u0)
    hit = np.zeros(U.P4, bool)
    for p, _, _, rec in flips:
        hit[p] = rec[0] < 4
    assert 0 < int(hit.sum()) < len(flips)
    for p in np.flatnonzero(hit):
        assert _refused(res1[p], res0[p]), (p, res1[p], res0[p])
    assert np.array_equal(res1[~hit], res0[~hit])
    want = out0.copy()
    for p in np.flatnonzero(hit):  # a refused request's range of a host output is left as it was
        want[int(res0["out_pos"][p]):int(res0["out_pos"][p]) + int(res0["bytes"][p])] = FILL
    assert np.array_equal(out1, want)
    return res1, out1


def test_many_partitions_fetch_verify(state4):
    e, cfg = state4
    clean = _fetch4(e, 0)
    rc0, res0, out0, u0 = clean
    assert rc0 == OK and (res0["status"] == 0).all() and u0 == int(res0["bytes"].sum()) <= 1 << 21
    assert np.array_equal(res0["count"], np.minimum(U.counts4(), 4))
    rc1, res1, out1, u1 = _fetch4(e, V)
    assert (rc1, u1) == (rc0, u0) and np.array_equal(res1, res0) and np.array_equal(out1, out0)
    # records 1, 6, 2, 7, 3, 8, 4, 9: those from the fourth on lie past their partition's slice of four
    flips = _marked_flips(e, cfg, (0,), index=lambda k: 1 + k // 2 + 5 * (k % 2))
    _assert_fetch4(e, flips, clean)
    rc1, res1, out1, u1 = _fetch4(e, V)
    assert np.array_equal(res1, res0) and np.array_equal(out1, out0)


# ---------------------------------------------------------------------------------------------
# the grid-stride loops
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def state1():
    e, cfg = _state1()
    yield e, cfg
    e.close()


P1, NC1 = 8, 4


def _all1(mx, flags):
    return _reqs(np.repeat(np.arange(P1), NC1), np.tile(np.arange(NC1), P1), mx, flags)


def _holders(e, cfg, p, rec_off, mx):
    """Consumers of partition p whose next slice of mx records holds offset rec_off."""
    offs = e.consumer_offsets(p)
    return [c for c in range(cfg.max_consumers) if int(offs[c]) <= rec_off < int(offs[c]) + mx]


@pytest.mark.parametrize("wgs", ["1", "3"])
def test_audit_grid_cap_state1(state1, monkeypatch, wgs):
    # the default grid's engine was created before the cap is set (read at rmq_create)
    d, cfg = state1
    monkeypatch.setenv("RMQ_AUDIT_WGS", wgs)
    e, _ = _state1()
    try:
        S = cfg.segment_bytes
        # one workgroup is 4 waves of 64 tasks: more tasks than a pass of it
        assert U.scrub_tasks(e.states(), cfg) > 256
        clean = d.scrub()
        U.assert_clean(clean, d, cfg)
        assert np.array_equal(e.scrub(), clean)
        for what in ("payload", "padding", "crc", "offset", "len_low", "len_top", "straddle", "first", "last"):
            p = 0 if what == "straddle" else 3
            recs = U.host_walk(d, cfg, 2, p)[2]
            rec, delta, mask = _pick(recs, S, what)
            ring_off = (rec[1] + delta) % S
            rows = []
            for x in (d, e):
                x.fault_flip_ring(2, p, ring_off, mask)
                try:
                    rows.append(x.scrub())
                    bad = U.host_walk(x, cfg, 2, p)[1]
                finally:
                    x.fault_flip_ring(2, p, ring_off, mask)
                assert bad == rec[0], (what, bad, rec)
            assert np.array_equal(rows[0], rows[1]), (what, rows)
            assert _scrub_row(rows[1][p]) == (ECORRUPT, rec[0], 2) and int(rows[1][p]["bad_kind"]) in KINDS[what], (what, rows[1][p])
        assert np.array_equal(e.scrub(), clean)
        # a 32-request flagged ticket, one slice flipped: 8 passes of the one workgroup's 4 waves
        p, mx = 3, 10
        recs = U.host_walk(d, cfg, 0, p)[2]
        rec = next(x for x in recs if x[2] == 600)
        hold = _holders(d, cfg, p, rec[0], mx)
        assert hold and len(hold) < NC1 and hold == _holders(e, cfg, p, rec[0], mx)
        res = []
        for x in (d, e):
            rc0, res0, out0, u0 = _call(x, _all1(mx, 0), 1 << 17)
            x.fault_flip_ring(0, p, (rec[1] + 16 + 300) % S)
            try:
                rc1, res1, out1, u1 = _call(x, _all1(mx, V), 1 << 17)
            finally:
                x.fault_flip_ring(0, p, (rec[1] + 16 + 300) % S)
            assert (rc1, u1) == (rc0, u0) == (OK, int(res0["bytes"].sum()))
            hit = np.zeros(P1 * NC1, bool)
            hit[[p * NC1 + c for c in hold]] = True
            for k in np.flatnonzero(hit):
                assert _refused(res1[k], res0[k]), (k, res1[k])
            assert np.array_equal(res1[~hit], res0[~hit])
            res.append((res1, out1))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    finally:
        e.close()


@pytest.mark.parametrize("wgs", ["1", "3"])
def test_audit_grid_cap_state4(state4, monkeypatch, wgs):
    d, cfg = state4
    monkeypatch.setenv("RMQ_AUDIT_WGS", wgs)
    e, _ = _state4()
    try:
        assert U.scrub_tasks(e.states(), cfg) > 3 * 256
        clean = d.scrub()
        U.assert_clean_bulk(clean, d.states(), 2)
        assert np.array_equal(e.scrub(), clean)
        flips = _marked_flips(d, cfg, (0, 1))
        rows = []
        for x in (d, e):
            _flip_all(x, flips)
            try:
                rows.append(x.scrub())
            finally:
                _flip_all(x, flips)
        assert _assert_marked_rows(rows[0], 0, flips, clean) == 8
        assert np.array_equal(rows[0], rows[1])
        assert np.array_equal(e.scrub(), clean)
        # the flagged 2500-row ticket: 625 passes of one workgroup
        fl = _marked_flips(d, cfg, (0,), index=lambda k: 1 + k // 2 + 5 * (k % 2))
        clean_f = _fetch4(d, 0)
        a = _assert_fetch4(d, fl, clean_f)
        b = _assert_fetch4(e, fl, clean_f)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    finally:
        e.close()


def test_fetch_verify_ticket_past_the_grid(state1):
    """A ticket of more requests than the verify grid has waves (8 workgroups per CU, 4 waves each):
    the waves' second pass checks, and refuses, like the first."""
    e, cfg = state1
    S = cfg.segment_bytes
    cus = e.device_info()[1]
    grid = 8 * cus * 4
    n = grid + 37
    combos = np.arange(n) % (P1 * NC1)
    pidx, cons = combos // NC1, combos % NC1
    cap = 1 << 23
    rc0, res0, out0, u0 = _call(e, _reqs(pidx, cons, 1, 0), cap)
    assert rc0 == OK and u0 == int(res0["bytes"].sum()) <= cap and (res0["status"] == 0).all()
    rc1, res1, out1, u1 = _call(e, _reqs(pidx, cons, 1, V), cap)
    assert (rc1, u1) == (rc0, u0) and np.array_equal(res1, res0) and np.array_equal(out1, out0)
    # the next record of (partition 0, consumer 2): rows 2, 34, ..., one of them past the first stride
    p, c = 0, 2
    off = int(e.consumer_offsets(p)[c])
    rec = next(x for x in U.host_walk(e, cfg, 0, p)[2] if x[0] == off)
    hold = _holders(e, cfg, p, off, 1)
    ring_off = (rec[1] + (16 + rec[2] // 2 if rec[2] else 12)) % S
    e.fault_flip_ring(0, p, ring_off)
    try:
        rc2, res2, out2, u2 = _call(e, _reqs(pidx, cons, 1, V), cap)
    finally:
        e.fault_flip_ring(0, p, ring_off)
    hit = (pidx == p) & np.isin(cons, hold)
    assert hit[2] and hit[grid:].any() and int(res0["count"][2]) == 1
    assert (rc2, u2) == (rc0, u0)
    for k in np.flatnonzero(hit):
        assert _refused(res2[k], res0[k]), (k, res2[k], res0[k])
    assert np.array_equal(res2[~hit], res0[~hit])
    want = out0.copy()
    for k in np.flatnonzero(hit):
        want[int(res0["out_pos"][k]):int(res0["out_pos"][k]) + int(res0["bytes"][k])] = FILL
    assert np.array_equal(out2, want)
    rc1, res1, out1, u1 = _call(e, _reqs(pidx, cons, 1, V), cap)
    assert np.array_equal(res1, res0) and np.array_equal(out1, out0)


# ---------------------------------------------------------------------------------------------
# the position cache after a refusal
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("repaired", [True, False])
def test_position_cache_after_a_refusal(oracle_mod, repaired):
    """A refused slice leaves no position-cache entry behind (FORMAT.md §10): the resolve wrote one
    from the damaged length words, and a consumer that skips the slice by committing start + count
    would otherwise start its next walk inside a record."""
    e, o, cfg = _state1(oracle_mod)
    try:
        S, p, c, mx = cfg.segment_bytes, 3, 1, 6
        start = int(e.consumer_offsets(p)[c])
        recs = U.host_walk(e, cfg, 0, p)[2]
        rec = next(x for x in recs if x[2] == 241)
        assert start <= rec[0] < start + mx and recs[-1][0] >= start + mx + 2  # in the slice; records follow it
        one = _reqs([p], [c], mx, V)
        rc0, res0, _, _ = _call(e, one, 1 << 16)
        assert rc0 == OK and (int(res0["status"][0]), int(res0["count"][0]), int(res0["start_offset"][0])) == (0, mx, start)
        ring_off = (rec[1] + 8) % S
        e.fault_flip_ring(0, p, ring_off, 0x01)  # 241 -> 240: the record ends a piece early for the walk
        flipped = True
        try:
            rc1, res1, _, _ = _call(e, one, 1 << 16)
            assert rc1 == OK and (int(res1["status"][0]), int(res1["count"][0])) == (ECORRUPT, 0), res1
            if repaired:
                e.fault_flip_ring(0, p, ring_off, 0x01)
                flipped = False
            _commit((e, o), [p], [c], [start + mx])  # the consumer skips the refused slice
            pidx, cons, mxs = np.array([p]), np.array([c]), np.array([mx])
            rco, reso, bo, uo = o.fetch(pidx, cons, mxs)
            assert rco == OK and int(reso["count"][0]) >= 2 and int(reso["start_offset"][0]) == start + mx
            for verify in (True, False):
                rc2, res2, b2, u2 = e.fetch(pidx, cons, mxs, out_cap=1 << 16, verify=verify)
                assert (rc2, u2) == (rco, uo) and np.array_equal(res2, reso), (verify, res2, reso)
                assert np.array_equal(b2[:u2], bo[:uo]), verify
        finally:
            if flipped:
                e.fault_flip_ring(0, p, ring_off, 0x01)
        U.assert_clean(e.scrub(), e, cfg)
    finally:
        e.close()
        o.close()


@pytest.mark.parametrize("case", ["refused", "refused_unrepaired", "enospc", "garbage"])
def test_position_cache_after_a_refusal_in_one_interval(oracle_mod, case):
    """The cases in which the cached position is wrong: short records, so that the slice's end lies
    in the index interval of the damaged length word and the resolve finds it by walking that word
    (above, the 241-byte record crosses an interval, the next entry names the record after it and
    the end is found from there). refused: the empty first record claims 32 bytes, exactly the
    record after it, so the walk stays on record starts and ends one record late; enospc: the same
    with an output the longer slice does not fit; garbage: the second record claims a piece more
    and the walk goes on through payload bytes. The consumer skips the slice; once the byte is
    repaired its next fetch is the oracle's. While the damage stays (refused_unrepaired), a lookup
    in that interval walks through it (FORMAT.md §5), so the flagged fetch is refused again, never
    served from a wrong position, and is the oracle's as soon as the byte is repaired."""
    e, o, cfg = _state1(oracle_mod)
    try:
        S, I, p, c, mx = cfg.segment_bytes, cfg.index_interval, 3, 0, 3
        start = int(e.consumer_offsets(p)[c])
        recs = U.host_walk(e, cfg, 0, p)[2]
        assert recs[0][0] == start and [x[2] for x in recs[:5]] == [0, 1, 15, 16, 17]
        rec, mask = (recs[1], 0x10) if case == "garbage" else (recs[0], 0x20)
        cap = 96 if case == "enospc" else 1 << 16
        assert rec[1] // I == recs[mx][1] // I  # no index entry between the damaged record and the slice's end
        one = _reqs([p], [c], mx, V)
        rc0, res0, _, u0 = _call(e, one, cap)
        assert rc0 == OK and (int(res0["status"][0]), int(res0["count"][0]), u0) == (0, mx, 80)
        ring_off = (rec[1] + 8) % S
        e.fault_flip_ring(0, p, ring_off, mask)
        flipped = True
        try:
            rc1, res1, _, _ = _call(e, one, cap)
            r = res1[0]
            assert int(r["count"]) == 0 and int(r["start_offset"]) == start, r
            if case == "enospc":
                assert rc1 == ENOSPC and int(r["status"]) == ENOSPC, (rc1, r)
            elif case == "garbage":
                assert int(r["status"]) in (ECORRUPT, ENOSPC), r
            else:  # the resolve walked the damaged word: the slice ends a record late
                assert rc1 == OK and (int(r["status"]), int(r["bytes"])) == (ECORRUPT, 80 + 32), r
            pidx, cons, mxs = np.array([p]), np.array([c]), np.array([mx])
            _commit((e, o), [p], [c], [start + mx])  # the consumer skips the slice
            rco, reso, bo, uo = o.fetch(pidx, cons, mxs)
            assert rco == OK and int(reso["count"][0]) == mx and int(reso["start_offset"][0]) == start + mx
            if case == "refused_unrepaired":
                rc2, res2, _, _ = e.fetch(pidx, cons, mxs, out_cap=1 << 16, verify=True)
                assert rc2 == OK and (int(res2["status"][0]), int(res2["count"][0])) == (ECORRUPT, 0), res2
            e.fault_flip_ring(0, p, ring_off, mask)
            flipped = False
            for verify in (True, False):
                rc2, res2, b2, u2 = e.fetch(pidx, cons, mxs, out_cap=1 << 16, verify=verify)
                assert (rc2, u2) == (rco, uo) and np.array_equal(res2, reso), (verify, res2, reso)
                assert np.array_equal(b2[:u2], bo[:uo]), verify
        finally:
            if flipped:
                e.fault_flip_ring(0, p, ring_off, mask)
        U.assert_clean(e.scrub(), e, cfg)
    finally:
        e.close()
        o.close()
