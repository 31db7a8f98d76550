"""The kernels at offsets and logical positions past 2^31, 2^32, 2^53 and 2^58.

rmq_restore with an empty run puts each partition of an engine at its own base
(high_base_util.bases_for: one stays at (0, 0) as the control); the ordinary append, fetch, audit,
ring-move, quorum and replication paths then run there. Every expected value is the CPU oracle's,
run from (0, 0) and translated by high_base_util.Translated in Python integers; that translation
and the edges these scenarios reach are pinned on the CPU by tests/test_high_base_model.py. The
device at a low base is never the reference.
"""
import ctypes as C

import numpy as np
import pytest

import fetch_budget_util as FB
import high_base_util as H
import scrub_util as U
from device_batch_util import DeviceBatch, append_device_checked
from parity import compare_index_slots, compare_state, ring_window, run_ops
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, LocalHub
from test_gpu_fetch_verify import _commit_offsets
from test_gpu_scrub import _run_ranks
from world_script import run_gpu, run_oracle

pytestmark = pytest.mark.gpu

OK, ECORRUPT = A.RMQ_OK, A.RMQ_ECORRUPT


@pytest.fixture()
def pair(oracle_mod):
    """pair(**cfg) -> (cfg, bases, rebased engine, translated oracle); closed after the test."""
    made = []

    def _pair(**kw):
        cfg = H.cfg_high(**kw)
        bases = H.bases_for(cfg.index_interval)
        dev = Engine(cfg)
        made.append(dev)
        t = H.Translated(oracle_mod.OracleEngine(cfg), cfg, bases)
        made.append(t)
        H.rebase(dev, bases, t)
        compare_state(dev, t, cfg)  # empty logs at their bases: state, E[dP / I], consumer rows
        return cfg, bases, dev, t

    yield _pair
    for x in made:
        x.close()


def _fill(dev, t, cfg, batches=4):
    """first_batch and `batches` scenario batches on both. With four, about 85 KB per partition:
    every 64 KiB ring has wrapped and every retained record lies above its partition's boundary."""
    ops = [("append", H.first_batch())] + [("append", b) for b in H.scenario_batches(batches)]
    run_ops(dev, t, cfg, ops, check=False)
    compare_state(dev, t, cfg)
    for p in range(cfg.num_partitions if batches >= 4 else 0):
        assert t.ora.state(p)["log_start_offset"] > 0, (p, "retention has run")


# ---- append
@pytest.mark.parametrize("depth,interval", [(1, 256), (2, 256), (3, 256), (2, 1024)])
def test_append_parity(pair, depth, interval):
    """Offsets, stats, state, windows and index after every step of high_base_util.scenario_ops
    (single appends, launch groups of `depth`, fetches between them) through several ring wraps.
    Depth 2 gives icap = 6 S / I, not a power of two: m mod icap at m = 2^23 .. 2^50."""
    cfg, bases, dev, t = pair(pipeline_depth=depth, index_interval=interval)
    run_ops(dev, t, cfg, H.scenario_ops(bases, depth))
    U.assert_clean(dev.scrub(), dev, cfg)


MODES = [{"RMQ_S3_ROLES": "0"}, {"RMQ_S3_ROLES": "1"}, {"RMQ_S3_ROLES": "4"}, {"RMQ_WG3_ALL": "0"}]


@pytest.mark.parametrize("env", MODES, ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_append_dispatch_modes(pair, monkeypatch, env):
    """The stage 3 dispatch modes test_gpu_parity.py runs (read at rmq_create), host batches."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, bases, dev, t = pair()
    b = H.scenario_batches(6)
    run_ops(dev, t, cfg, [("append", H.first_batch())] + [("pipelined", b[k:k + 2]) for k in (0, 2, 4)])


def test_append_device_batches(pair):
    """The same batches from device memory (RMQ_MEM_DEVICE), the payload 4 bytes off a 16-byte line."""
    cfg, bases, dev, t = pair()
    for k, b in enumerate([H.first_batch()] + H.scenario_batches(5)):
        db = DeviceBatch(dev, b, shift=(0, 4)[k % 2])
        sd = append_device_checked(dev, t, db, what=f"batch {k}")
        assert sd["appended"] == b.n, sd
        db.free()
        compare_state(dev, t, cfg)


# ---- fetch
def _reqs(cfg):
    nc = cfg.max_consumers
    return np.repeat(np.arange(cfg.num_partitions), nc), np.tile(np.arange(nc), cfg.num_partitions)


def _same_fetch(got, want, what=""):
    rc, res, buf, used = got
    rc0, res0, buf0, used0 = want
    assert (rc, used) == (rc0, used0), (what, rc, used, rc0, used0)
    bad = np.flatnonzero(res != res0)
    assert bad.size == 0, (what, bad[:4], res[bad[:4]], res0[bad[:4]])
    n = min(used, len(buf))
    assert np.array_equal(buf[:n], buf0[:n]), (what, "fetched bytes differ")


def test_fetch_index_search_and_row_kinds(pair):
    """Cold consumers (no position cache: the sparse-index search and its interpolated start) at
    the log start, inside, near the end and at the end of every partition, max 1, 10 and 1024; an
    output too small (capacity RMQ_ENOSPC); consumers below the log start (RMQ_EOFFSET) and beyond
    the high watermark, one of them 2^32 past the base."""
    cfg, bases, dev, t = pair()
    _fill(dev, t, cfg)
    for e in (dev, t):
        _commit_offsets(e, cfg)
    pidx, cons = _reqs(cfg)
    n = len(pidx)
    ops = [("fetch", pidx, cons, np.full(n, mx, np.uint32)) for mx in (1, 10, 1024)]
    ops.append(("fetch", pidx, cons, np.full(n, 1024, np.uint32), 5000))
    pp = np.arange(8, dtype=np.uint32)
    st = [t.state(int(p)) for p in pp]
    below = np.array([bases[int(p)][0] + 1 for p in pp], np.uint64)          # evicted
    past = np.array([bases[int(p)][0] + 2 ** 32 for p in pp], np.uint64)     # far beyond the log end
    edge = np.array([s["high_watermark"] + 1 for s in st], np.uint64)
    for c, offs in enumerate((below, past, edge)):
        ops.append(("consumer_commit", pp, np.full(8, c, np.uint32), offs))
    ops += [("fetch", pidx, cons, np.full(n, 7, np.uint32)), ("fetch", pidx, cons, np.full(n, 0xFFFFFFFF, np.uint32))]
    log = run_ops(dev, t, cfg, ops, check=False)
    seen = {int(s) for kind, res, _ in log for s in res["status"]}
    assert {OK, A.RMQ_EOFFSET, A.RMQ_ENOSPC} <= seen, seen
    compare_state(dev, t, cfg)


@pytest.mark.parametrize("mx", [10, 33])
def test_fetch_read_then_commit_loop(pair, mx):
    """The consume loop: read mx, commit start + count, until drained; from the second read on the
    position cache serves it (mx 10) or, past kWalkMax = 32 records, the index search does (mx 33).
    Consumer 1 does the same with RMQ_FETCH_COMMIT."""
    cfg, bases, dev, t = pair()
    _fill(dev, t, cfg, 2)
    pp = np.arange(8, dtype=np.uint32)
    for e in (dev, t):
        lo = np.array([e.state(int(p))["log_start_offset"] for p in pp], np.uint64)
        for c in (0, 1):
            e.commit_consumer_offset(pp, np.full(8, c, np.uint32), lo)
    for k in range(12):
        got = []
        for e in (dev, t):
            r = e.fetch(pp, np.zeros(8, np.uint32), np.full(8, mx, np.uint32))
            nxt = [int(a) + int(b) for a, b in zip(r[1]["start_offset"], r[1]["count"])]
            e.commit_consumer_offset(pp, np.zeros(8, np.uint32), np.array(nxt, np.uint64))
            got.append(r)
        _same_fetch(*got, what=f"read {k}")
        got = [e.fetch(pp, np.ones(8, np.uint32), np.full(8, mx, np.uint32), commit=True) for e in (dev, t)]
        _same_fetch(*got, what=f"read and commit {k}")
        assert (got[0][1]["status"] == OK).all()
    compare_state(dev, t, cfg)
    assert all(int(t.ora.consumer_offsets(p)[0]) > 0 for p in range(8))


def test_fetch_budgets_verify_and_async(pair):
    """rmq_fetch_bytes against fetch_budget_util's model fed the translated slices; RMQ_FETCH_VERIFY
    on clean logs; one asynchronous ticket into device memory with page-locked rows, one with rows in
    device memory, and a synchronous call with device rows."""
    cfg, bases, dev, t = pair()
    _fill(dev, t, cfg)
    for e in (dev, t):
        _commit_offsets(e, cfg)
    pidx, cons = _reqs(cfg)
    n = len(pidx)
    cats = set()
    for mx in (10, 1024):
        for b in (16, 17, 255, 272, 1520, 4096, 0xFFFFFFFF):
            want = FB.model_fetch(t, pidx, cons, mx, b)
            FB.assert_equals_model(dev.fetch(pidx, cons, np.full(n, mx), max_bytes=b), want, (mx, b))
            cats |= set(want[4])
    assert {"zero", "one", "mid", "untrimmed", "empty"} <= cats, cats
    want = t.fetch(pidx, cons, np.full(n, 10))
    _same_fetch(dev.fetch(pidx, cons, np.full(n, 10), verify=True), want, "verify")
    cap = 1 << 18
    assert want[3] <= cap
    d_out = dev.device_alloc(cap)
    got = np.empty(cap, np.uint8)
    # page-locked rows, asynchronous
    req, res = dev.fetch_rows(n)
    req[:, 0], req[:, 1], req[:, 2] = pidx, cons, 10
    rc, rows, used = dev.fetch_poll(dev.fetch_async(None, None, None, d_out=d_out, out_cap=cap, req=req, res=res,
                                                    pinned_rows=True), wait=True)
    dev.d2h(got, d_out)
    _same_fetch((rc, rows, got, used), want, "async, pinned rows")
    # device rows, asynchronous (the raw call: Engine.fetch_async takes host rows) and synchronous
    d_req, d_res = dev.device_alloc(16 * n), dev.device_alloc(FETCH_RES_DTYPE.itemsize * n)
    dev.h2d(d_req, np.ascontiguousarray(req))
    for asyn in (True, False):
        dev.h2d(d_out, np.zeros(cap, np.uint8))
        dev.h2d(d_res, np.zeros(n, FETCH_RES_DTYPE))
        if asyn:
            tk, u = C.c_uint64(), C.c_uint64()
            rc = dev.lib.rmq_fetch_async(dev.h, C.c_void_p(d_req), n, A.RMQ_MEM_DEVICE | A.RMQ_FETCH_DEVICE_ROWS,
                                         C.c_void_p(d_out), cap, C.c_void_p(d_res), C.byref(tk))
            assert rc == OK, rc
            rc = dev.lib.rmq_fetch_poll(dev.h, tk.value, 1, C.byref(u))
            used = int(u.value)
        else:
            rc, _, used = dev.fetch_device(None, None, None, d_out, cap, d_rows=(n, d_req, d_res))
        rows = np.empty(n, FETCH_RES_DTYPE)
        dev.d2h(rows, d_res)
        dev.d2h(got, d_out)
        _same_fetch((rc, rows, got, used), want, f"device rows, async={asyn}")
    for d in (d_out, d_req, d_res):
        dev.device_free(d)


# ---- audit
def _record_above(t, cfg, p):
    """(offset, logical position, payload length) of a retained record of p with a payload, two
    thirds into the window: above the partition's boundary in offset and position."""
    recs = [r for r in H.window_records(t, cfg, p) if r[2] >= 4]
    return recs[2 * len(recs) // 3]


AUDITED = (1, 2, 3, 4, 5)  # one partition of every base


def test_scrub_repair_and_verified_fetch_name_the_record(pair):
    """A clean scrub; a payload byte of one record per base flipped on slot 0: the scrub and a
    verified fetch name that record's offset, which is where the host walk over the bytes read back
    stops; rmq_repair restores the window from another slot and the scrub is clean again."""
    cfg, bases, dev, t = pair()
    _fill(dev, t, cfg)
    S = cfg.segment_bytes
    U.assert_clean(dev.scrub(), dev, cfg)
    want = {}
    for p in AUDITED:
        off, pos, ln = _record_above(t, cfg, p)
        assert off > bases[p][0] and pos > bases[p][1] and off > H.CROSSING.get(p, 0) and pos > H.CROSSING.get(p, 0)
        dev.fault_flip_ring(0, p, (pos + 16 + ln // 2) % S, 0x5A)
        assert U.host_walk(dev, cfg, 0, p)[1] == off, (p, off)  # the host walk stops at that record
        want[p] = off
    rows = dev.scrub()
    assert dev.last_scrub_rc == ECORRUPT
    for p in range(8):
        r = rows[p]
        if p in want:
            assert (int(r["status"]), int(r["bad_offset"]), int(r["bad_replica"]), int(r["bad_kind"])) == \
                (ECORRUPT, want[p], 0, A.RMQ_SCRUB_BAD_CRC), (p, r, want[p])
        else:
            assert int(r["status"]) == OK and int(r["bad_offset"]) == U.NONE, (p, r)
    # a verified fetch of that record alone, and of the record before it
    pp = np.array(AUDITED, np.uint32)
    for c, d in ((0, 0), (1, 1)):
        offs = np.array([want[int(p)] - d for p in pp], np.uint64)
        for e in (dev, t):
            e.commit_consumer_offset(pp, np.full(len(pp), c, np.uint32), offs)
    pidx, cons = np.repeat(pp, 2), np.tile(np.array([0, 1], np.uint32), len(pp))
    rc, res, buf, used = dev.fetch(pidx, cons, np.ones(len(pidx), np.uint32), verify=True)
    rc0, res0, buf0, used0 = t.fetch(pidx, cons, np.ones(len(pidx), np.uint32))
    assert (res0["count"] == 1).all()
    exp = res0.copy()
    exp["status"][cons == 0], exp["count"][cons == 0] = ECORRUPT, 0  # start_offset, out_pos and bytes stay
    assert (rc, used) == (rc0, used0) and np.array_equal(res, exp), (res, exp)
    assert [int(x) for x in res["start_offset"][cons == 0]] == [want[int(p)] for p in pp]
    for r in np.flatnonzero(cons == 1):
        lo, hi = int(res["out_pos"][r]), int(res["out_pos"][r]) + int(res["bytes"][r])
        assert np.array_equal(buf[lo:hi], buf0[lo:hi]), r
    rep = dev.repair()
    assert dev.last_repair_rc == OK
    for p in range(8):
        assert int(rep[p]["segments_repaired"]) == (1 if p in want else 0), (p, rep[p])
        assert int(rep[p]["segments_unrepaired"]) == 0 and int(rep[p]["status"]) == OK, (p, rep[p])
    compare_state(dev, t, cfg)
    U.assert_clean(dev.scrub(), dev, cfg)


@pytest.mark.parametrize("depth", [2, 3])
def test_reindex_rewrites_a_flipped_entry(pair, depth):
    """One live index entry per base flipped (the offset word's bit 33, the position word's bit 4):
    the scrub fails, rmq_reindex rewrites exactly those entries to the translated oracle's, and the
    scrub is clean. The entry's slot is m mod icap with m = 2^23 .. 2^50; depth 2: icap = 6 S / I."""
    cfg, bases, dev, t = pair(pipeline_depth=depth)
    _fill(dev, t, cfg)
    I = cfg.index_interval
    for p in AUDITED:
        st = t.state(p)
        m_lo, m_hi = -(-st["log_start_pos"] // I), st["log_end_pos"] // I
        m = (m_lo + 2 * m_hi) // 3
        assert m * I > H.CROSSING.get(p, 0) and m >= bases[p][1] // I
        dev.fault_flip_index(p, m, p % 2, (1 << 33, 1 << 4)[p % 2])
    rows = dev.scrub()
    assert all(int(rows[p]["status"]) == ECORRUPT and int(rows[p]["bad_kind"]) == A.RMQ_SCRUB_BAD_CHAIN for p in AUDITED), rows
    out = dev.reindex()
    assert dev.last_reindex_rc == OK
    for p in range(8):
        assert int(out[p]["entries_rewritten"]) == (1 if p in AUDITED else 0), (p, out[p])
        assert int(out[p]["gaps_unresolved"]) == 0 and int(out[p]["status"]) == OK, (p, out[p])
    compare_state(dev, t, cfg)
    U.assert_clean(dev.scrub(), dev, cfg)


# ---- ring moves
def _move(dev, t, cfg, pidx, sizes):
    """One rmq_set_segments on both; state, windows and live entries, then every slot of the moved
    partitions' index rings (a move leaves {0, 0} outside the live range)."""
    run_ops(dev, t, cfg, [("set_segments", np.array(pidx, np.uint32), np.array(sizes, np.uint64))])
    for p in pidx:
        compare_index_slots(dev, t, cfg, p)


def test_ring_moves_of_windows_that_straddle_the_boundary(pair):
    """rmq_set_segments grows and shrinks partitions whose window [log_start_pos, log_end_pos) holds
    2^32 (2^31): the window is copied to pos mod S', the live index entries move to m mod icap'.
    Then appends, a shrink with retention (m* = ceil((log_end_pos - S') / I)) and a shrink back."""
    cfg, bases, dev, t = pair(pool_bytes=4 * 8 * (1 << 16))
    S = cfg.segment_bytes
    b = H.scenario_batches(5, config_index=75)
    run_ops(dev, t, cfg, [("append", H.first_batch())])
    _move(dev, t, cfg, [1, 3, 6, 2, 5], [2 * S, 4096, 4 * S, 2 * S, 8192])
    for p in H.CROSSING:  # still astride after the move
        st = t.state(p)
        assert st["log_start_pos"] < H.CROSSING[p] < st["log_end_pos"], (p, st)
    run_ops(dev, t, cfg, [("append", b[0]), ("append", b[1])])
    _move(dev, t, cfg, [1, 6, 4], [8192, S, 4096])  # 1 and 4: retention at the new size first
    assert t.ora.state(1)["log_start_offset"] > 0 and t.ora.state(4)["log_start_offset"] > 0
    run_ops(dev, t, cfg, [("pipelined", b[2:4])])
    _move(dev, t, cfg, [3, 5], [S, S])
    run_ops(dev, t, cfg, [("append", b[4]), ("fetch", np.arange(8), np.zeros(8), np.full(8, 1024))])
    U.assert_clean(dev.scrub(), dev, cfg)


# ---- quorum
def test_quorum_acks_on_both_sides_of_the_boundary(pair):
    """high_base_util.quorum_ops: one or two slots remote, rmq_ack with match values below and above
    2^32, of exactly 2^31, beyond the log end (clamped to it) and up to 2^59; commit and
    high_watermark follow the oracle's after every ack, and a fetch is bounded by them."""
    cfg, bases, dev, t = pair()
    ops = [("append", H.first_batch())] + H.quorum_ops(bases) + [("append", H.scenario_batches(1, config_index=76)[0])]
    run_ops(dev, t, cfg, ops, local_slots=H.local_slots_of(dev))
    st = dev.state(1)
    assert st["replica_rank"] == [0, 1, 2] and st["commit"] > 2 ** 32 and st["commit"] == st["match"][1]


# ---- replication
def test_world_of_three_at_high_bases(oracle_mod):
    """Three engines over the local hub, every rank rebased to the same bases before it attaches;
    high_base_util.world_steps (rounds with appends, a consumer commit, a round that rank 1 misses and
    its catch-up) through world_script. Every rank's states (led and followed), windows of the slots
    it holds, live index entries and consumer rows equal the translated oracle world's. The only leg
    that takes ingest, acks and commit notices past 2^32 and to 2^58."""
    views, cfgs, bases = H.world_setup()
    zero = [{p: (0, 0) for p in b} for b in bases]
    hub, engs, oras = LocalHub(H.WORLD), [Engine(c) for c in cfgs], [oracle_mod.OracleEngine(c) for c in cfgs]
    try:
        for r in range(H.WORLD):
            H.rebase(engs[r], bases[r], oras[r])
        got = run_gpu(engs, hub, views, H.world_steps(views, bases), timeout=60)
        want = run_oracle(oras, views, H.world_steps(views, zero))
        assert all(s == OK for r in range(H.WORLD) for s in got[0][r]) and got[0] == want[0]
        for r in range(H.WORLD):
            cfg = cfgs[r]
            t = H.Translated(oras[r], cfg, bases[r])
            for k, step in enumerate(H.world_steps(views, bases)):
                if step[0] == "commit":
                    assert got[k][r][0] == want[k][r][0] and np.array_equal(got[k][r][1], want[k][r][1]), (k, r)
                if step[0] == "fetch":
                    rc0, res0, buf0 = want[k][r]
                    buf0 = buf0.copy()
                    res0 = t.fetch_up(step[1][r][0], res0, buf0)
                    rc, res, buf = got[k][r]
                    assert rc == rc0 and np.array_equal(res, res0) and np.array_equal(buf, buf0), (k, r, res, res0)
                    assert (res["count"] > 0).all() or k > 4  # (the later fetch is RMQ_EOFFSET)
            for p in range(cfg.num_partitions):
                sg, so = H.follower_view(engs[r].state(p), r), H.follower_view(t.state(p), r)
                assert sg == so, f"rank {r} partition {p} (global {int(views[r].gp[p])})\n gpu={sg}\n cpu={so}"
            held = H.local_slots_of(engs[r])
            for p in range(cfg.num_partitions):
                st = t.state(p)
                for s in held(p):
                    a, b = ring_window(engs[r], cfg, s, p, st), ring_window(t, cfg, s, p, st)
                    assert np.array_equal(a, b), (r, p, s, np.flatnonzero(a != b)[:4])
                I = cfg.index_interval
                m_lo, m_hi = -(-st["log_start_pos"] // I), st["log_end_pos"] // I
                assert np.array_equal(engs[r].read_index(p, m_lo, m_hi - m_lo + 1), t.read_index(p, m_lo, m_hi - m_lo + 1)), (r, p)
                assert np.array_equal(engs[r].consumer_offsets(p), t.consumer_offsets(p)), (r, p)
            stats = engs[r].replication_stats()
            assert stats["records_ingested"] > 0 and stats["refused_crc"] == 0, (r, stats)
        assert engs[0].replication_stats()["catchup_entries"] > 0, "rank 1 missed a round of rank 0"

        def audit(r):  # collective: led and followed partitions alike
            rows = engs[r].scrub()
            assert engs[r].last_scrub_rc == OK and (rows["status"] == OK).all(), (r, rows)

        _run_ranks(H.WORLD, audit)
    finally:
        for o in oras:
            o.close()
        for e in engs:
            e.close()
        hub.close()
