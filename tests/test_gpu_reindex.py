"""rmq_reindex on the GPU (FORMAT.md §10, "Index rebuild"): single flips, runs and several gaps, the
large records of state 2, many partitions, the edge shapes of the live range, the slot switch,
unresolved gaps, the dry run, RMQ_REINDEX_ALL, clean logs, life after a rebuild, followers over a
transport, and the refusals. Every expected entry and counter comes from the host model
(tests/reindex_util.py, checked on the CPU by tests/test_reindex_model.py) over bytes read back
before the damage, never from rmq_reindex.

While an entry is damaged only rmq_scrub, rmq_repair, rmq_reindex and the read-back calls run: they
treat index words as data under containment checks. Nothing appends, fetches or moves rings then."""
import numpy as np
import pytest

import reindex_util as X
import repair_util as R
import scrub_util as U
from parity import run_ops
from repl_sim import leader_change_script, place, rank_cfg
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine, EngineConfig, EngineError, LocalHub
from ripplemq_amd.sharding import rank_view
from ripplemq_amd.workload import Batch, StreamSpec, make_batch
from test_gpu_scrub import _run_ranks

pytestmark = pytest.mark.gpu

OK, ECORRUPT = A.RMQ_OK, A.RMQ_ECORRUPT
ROW = ["bad_offset", "bad_replica", "bad_kind", "replicas", "status"]
OFF, POS = 0, 1
# an offset bit; a low pos bit (breaks the alignment); a high pos bit (outside the log: no bounds)
FLIPS = {"offset": (OFF, 1 << 1), "pos_low": (POS, 1 << 2), "pos_high": (POS, 1 << 40)}


@pytest.fixture()
def fresh1():
    with Engine(U.cfg1()) as e:
        U.fill1(e)
        yield e, U.cfg1()


@pytest.fixture(scope="module")
def state1():
    with Engine(U.cfg1()) as e:
        U.fill1(e)
        yield e, U.cfg1()


@pytest.fixture(scope="module")
def state2():
    with Engine(U.cfg2()) as e:
        U.fill2(e)
        yield e, U.cfg2()


def _counts(rows, first=0):
    return {first + i: (int(r["entries_live"]), int(r["entries_rewritten"]), int(r["gaps_unresolved"]))
            for i, r in enumerate(rows)}


def _same_rows(a, b):
    return all(np.array_equal(a[f], b[f]) for f in ROW)


def _assert_bytes(e, cfg, snap, what=""):
    """The live index and every ring byte of every slot of the snapshot's partitions."""
    I = cfg.index_interval
    for p, (st, ents, rs) in snap.items():
        lo, hi = X.live_range(st, I)
        if lo <= hi:
            got = e.read_index(p, lo, hi - lo + 1)
            assert np.array_equal(got, ents.reshape(-1, 2)), (what, p, lo, np.flatnonzero((got != ents).any(axis=1)))
        for r, a in rs.items():
            got = e.read_segment(r, p, 0, a.size)
            assert np.array_equal(got, a), (what, p, r, np.flatnonzero(got != a)[:8])


def _damage(e, changes, flips=()):
    for p, m, word, mask in changes:
        e.fault_flip_index(p, m, word, mask)
    for f in flips:
        e.fault_flip_ring(*f)


def _damaged(snap, I, changes, flips=()):
    bad = snap
    for p, m, word, mask in changes:
        bad = X.with_entries(bad, I, p, [(m, word, mask)])
    return R.apply_flips(bad, flips)


def _damage_and_reindex(e, cfg, changes, flips=(), parts=None, first=0, n=None, all_mode=False, dry=True, slots=None):
    """Snapshot, model, damage, (dry run,) reindex, scrub: the checks every scenario shares. changes:
    [(p, m, word, mask)] index words; flips: [(slot, p, ring offset, mask)] ring bytes. Returns
    (rows, return value, the following scrub's rows, the clean snapshot, the damaged one, the model)."""
    I = cfg.index_interval
    n = cfg.num_partitions - first if n is None else n
    snap = R.snapshot(e, cfg, parts, slots)
    states, cons = e.states(), e.consumer_table()
    bad = _damaged(snap, I, changes, flips)
    want = X.model({p: v for p, v in bad.items() if first <= p < first + n}, I, all_mode)
    want_counts = {p: w[1:] for p, w in want.items()}
    _damage(e, changes, flips)
    if dry:
        before = e.scrub(first, n)
        d = e.reindex(first, n, dry_run=True, all=all_mode)
        assert e.last_reindex_rc == e.last_scrub_rc
        got = _counts(d, first)
        assert {p: got[p] for p in want_counts} == want_counts, (got, want_counts)
        assert _same_rows(d, before)  # the present state: the scrub's row
        _assert_bytes(e, cfg, bad, "dry run")  # nothing written
    rows = e.reindex(first, n, all=all_mode)
    rc = e.last_reindex_rc
    after = e.scrub(first, n)
    assert rc == e.last_scrub_rc and _same_rows(rows, after), (rows, after)
    got = _counts(rows, first)
    assert {p: got[p] for p in want_counts} == want_counts, (got, want_counts)
    assert all(c[1:] == (0, 0) for p, c in got.items() if p not in want_counts)
    left = {p: (st, want[p][0] if p in want else ents, rs) for p, (st, ents, rs) in bad.items()}
    _assert_bytes(e, cfg, left, "reindex")  # the model's index; every ring byte as it was damaged
    assert np.array_equal(e.states(), states) and np.array_equal(e.consumer_table(), cons)
    return rows, rc, after, snap, bad, want


def _live(e, cfg, p):
    return X.live_range(e.state(p), cfg.index_interval)


def _walked_entry(e, cfg, p):
    """(m, pos): a live entry m whose predecessor names a record start below m * I, at pos: the walk
    of a gap at m starts on that record and has to accept it."""
    lo, hi = _live(e, cfg, p)
    ents = e.read_index(p, lo, hi - lo + 1)
    for m in range(lo + 3, hi - 3):
        if int(ents[m - 1 - lo][1]) < m * cfg.index_interval:
            return m, int(ents[m - 1 - lo][1])
    raise AssertionError("no such entry")


# ---- clean logs
@pytest.mark.parametrize("which", [1, 2])
def test_clean_logs(state1, state2, which):
    e, cfg = state1 if which == 1 else state2
    scrub = e.scrub()
    rows, rc, after, snap, _, want = _damage_and_reindex(e, cfg, [])
    assert rc == OK and _same_rows(rows, scrub) and all(w[2:] == (0, 0) for w in want.values())
    U.assert_clean(after, e, cfg)
    assert _counts(e.reindex(2, 3), 2) == {p: _counts(rows)[p] for p in (2, 3, 4)}  # a sub-range names the same partitions


# ---- single flips
@pytest.mark.parametrize("where", ["lo", "mid", "hi"])
@pytest.mark.parametrize("flip", list(FLIPS))
def test_single_flip(state1, where, flip):
    e, cfg = state1
    p = 2
    lo, hi = _live(e, cfg, p)
    m = {"lo": lo, "mid": (lo + hi) // 2, "hi": hi}[where]
    word, mask = FLIPS[flip]
    rows, rc, after, snap, _, _ = _damage_and_reindex(e, cfg, [(p, m, word, mask)])
    assert rc == OK and _counts(rows)[p] == (hi - lo + 1, 1, 0)
    assert int(rows["entries_rewritten"].sum()) == 1
    _assert_bytes(e, cfg, snap)  # the index equals the snapshot, nothing else moved
    U.assert_clean(after, e, cfg)


# ---- runs and several gaps
def _two_gaps(e, cfg, p):
    lo, hi = _live(e, cfg, p)
    assert hi - lo >= 8
    return [(p, lo + 2, POS, 1 << 2), (p, hi - 2, OFF, 1 << 4)]


def test_adjacent_entries_form_one_gap(state1):
    e, cfg = state1
    p = 1
    lo, hi = _live(e, cfg, p)
    m = lo + 4
    changes = [(p, m, OFF, 1), (p, m + 1, POS, 1 << 40), (p, m + 2, POS, 1 << 3)]
    bad = _damaged(R.snapshot(e, cfg, [p]), cfg.index_interval, changes)
    assert len(X.gaps_of(*bad[p], cfg.index_interval)[0]) == 1
    rows, rc, after, snap, _, _ = _damage_and_reindex(e, cfg, changes)
    assert rc == OK and _counts(rows)[p][1:] == (3, 0)
    _assert_bytes(e, cfg, snap)


def test_two_gaps_in_one_partition(state1):
    e, cfg = state1
    p = 3
    changes = _two_gaps(e, cfg, p)
    bad = _damaged(R.snapshot(e, cfg, [p]), cfg.index_interval, changes)
    assert len(X.gaps_of(*bad[p], cfg.index_interval)[0]) == 2
    rows, rc, after, snap, _, _ = _damage_and_reindex(e, cfg, changes)
    assert rc == OK and _counts(rows)[p][1:] == (2, 0)
    _assert_bytes(e, cfg, snap)


@pytest.mark.parametrize("wgs", [None, "1", "3"])
def test_two_gaps_in_every_active_partition(monkeypatch, wgs):
    if wgs:
        monkeypatch.setenv("RMQ_AUDIT_WGS", wgs)  # (read at rmq_create) twelve gaps over four waves: the stride loops run
    cfg = U.cfg1()
    with Engine(cfg) as e:
        U.fill1(e)
        changes = [c for p in range(U.ACTIVE1) for c in _two_gaps(e, cfg, p)]
        rows, rc, after, snap, _, _ = _damage_and_reindex(e, cfg, changes)
        assert rc == OK and [_counts(rows)[p][1:] for p in range(U.ACTIVE1)] == [(2, 0)] * U.ACTIVE1
        _assert_bytes(e, cfg, snap)
        U.assert_clean(after, e, cfg)


# ---- state 2: records over 64 pieces
def test_entry_inside_a_run_under_a_large_record(state2):
    e, cfg = state2
    I, S = cfg.index_interval, cfg.segment_bytes
    changes = []
    # the middle of the run of equal entries under a 9,000-byte record: empty segments, a walk that
    # starts beyond the damaged multiple
    for p in range(4):
        lo, hi = _live(e, cfg, p)
        ents = e.read_index(p, lo, hi - lo + 1)
        run = [k for k in range(2, len(ents) - 2) if all(np.array_equal(ents[k], ents[k + d]) for d in (-2, -1, 1, 2))]
        if run:
            changes.append((p, lo + run[0], POS, 1 << 5))
            break
    assert changes
    # an entry beside the record that wraps the ring end (another partition)
    for q in range(4):
        if q == changes[0][0]:
            continue
        recs = U.host_walk(e, cfg, 0, q)[2]
        wrap = [x for x in recs if x[1] // S != (x[1] + 16 + ((x[2] + 15) & ~15) - 1) // S]
        if wrap:
            lo, hi = _live(e, cfg, q)
            m = min(max(-(-wrap[0][1] // I), lo), hi)  # the first entry at or after the record's start
            changes.append((q, m, OFF, 1 << 2))
            break
    assert len(changes) == 2
    rows, rc, after, snap, _, _ = _damage_and_reindex(e, cfg, changes)
    assert rc == OK and [_counts(rows)[c[0]][1:] for c in changes] == [(1, 0), (1, 0)]
    _assert_bytes(e, cfg, snap)
    U.assert_clean(after, e, cfg)


# ---- state 4: 2,500 partitions, a sub-range
def test_many_partitions():
    cfg = U.cfg4()
    with Engine(cfg) as e:
        U.fill4(e)
        states = e.states()
        changes = []
        for k, p in enumerate(U.MARKED4):
            lo, hi = _live(e, cfg, p)
            assert hi > lo
            changes.append((p, lo + (k * (hi - lo)) // (len(U.MARKED4) - 1), k % 2, 1 << (3 + k)))
        near = [p for m in U.MARKED4 for p in (m - 1, m, m + 1) if 0 <= p < U.P4]
        # a sub-range that starts inside a plan chunk: 1023, 1024, 2047 and 2048 lie in it; the
        # damaged partitions outside it stay damaged and untouched
        rows, rc, after, snap, bad, _ = _damage_and_reindex(e, cfg, changes, parts=near, first=1000, n=1100)
        assert rc == OK and int(rows["entries_rewritten"].sum()) == 4 and not rows["gaps_unresolved"].any()
        U.assert_clean_bulk(after, states[1000:2100], 2)
        assert e.scrub(0, 1000)["status"][0] == ECORRUPT
        rows = e.reindex()
        assert e.last_reindex_rc == OK and int(rows["entries_rewritten"].sum()) == 4
        assert sorted(np.flatnonzero(rows["entries_rewritten"])) == [p for p in U.MARKED4 if not 1000 <= p < 2100]
        _assert_bytes(e, cfg, snap)
        U.assert_clean_bulk(e.scrub(), states, 2)
        assert np.array_equal(e.states(), states)


# ---- the edge shapes of the live range
def test_log_start_on_a_multiple_and_an_empty_log():
    cfg = U.cfg1()
    with Engine(cfg) as e:
        for _ in range(3):  # records of exactly one interval: the retained log starts on a multiple
            _, st = e.append(np.zeros(8, np.uint32), np.full(8, 240, np.uint32), np.arange(8 * 240, dtype=np.uint8))
            assert st["appended"] == 8
        st = e.state(0)
        lo, hi = _live(e, cfg, 0)
        assert st["log_start_pos"] > 0 and st["log_start_pos"] == lo * cfg.index_interval
        assert (e.state(1)["log_start_pos"], e.state(1)["log_end_pos"]) == (0, 0) and _live(e, cfg, 1) == (0, 0)
        changes = [(0, lo, OFF, 1), (1, 0, POS, 1 << 4)]
        rows, rc, after, snap, _, _ = _damage_and_reindex(e, cfg, changes)
        assert rc == OK and _counts(rows)[0] == (hi - lo + 1, 1, 0) and _counts(rows)[1] == (1, 1, 0)
        assert snap[0][1][0].tolist() == [st["log_start_offset"], st["log_start_pos"]]
        _assert_bytes(e, cfg, snap)
        U.assert_clean(after, e, cfg)


# ---- a record beside the entry is damaged on one slot: the walk switches slots
def test_slot_switch_then_repair(fresh1):
    e, cfg = fresh1
    I, S = cfg.index_interval, cfg.segment_bytes
    p = 4
    m, pos = _walked_entry(e, cfg, p)
    changes, flips = [(p, m, OFF, 1 << 2)], [(0, p, (pos + 12) % S, 0x5A)]
    rows, rc, after, snap, bad, _ = _damage_and_reindex(e, cfg, changes, flips)
    # the entry is rebuilt through slot 1; slot 0's record stays damaged, for rmq_repair
    assert rc == ECORRUPT and _counts(rows)[p][1:] == (1, 0) and int(after[p]["bad_replica"]) == 0
    healed = {q: (st, snap[q][1], rs) for q, (st, _, rs) in bad.items()}
    want_rings, want_counts = R.model(healed, I)
    assert want_counts[p] == (1, want_counts[p][1], 0)
    # (as the code stood the index damage stayed, and the repair's model leaves such a partition unrepaired)
    assert R.model(bad, I)[1][p][2] > 0
    rep = e.repair()
    assert e.last_repair_rc == OK
    assert (int(rep[p]["segments_repaired"]), int(rep[p]["bytes_repaired"]), int(rep[p]["segments_unrepaired"])) == want_counts[p]
    _assert_bytes(e, cfg, snap)
    U.assert_clean(e.scrub(), e, cfg)


# ---- a record damaged on every slot
def test_unresolved_gap_stays_and_another_resolves(fresh1):
    e, cfg = fresh1
    S = cfg.segment_bytes
    p = 5
    lo, hi = _live(e, cfg, p)
    m, pos = _walked_entry(e, cfg, p)
    assert hi - 1 > m + 2
    changes = [(p, m, OFF, 1 << 2), (p, hi - 1, POS, 1 << 3)]
    flips = [(r, p, (pos + 12) % S, 0x5A) for r in range(3)]
    rows, rc, after, snap, bad, want = _damage_and_reindex(e, cfg, changes, flips)
    assert rc == ECORRUPT and int(rows[p]["status"]) == ECORRUPT and _counts(rows)[p][1:] == (1, 1)
    got = e.read_index(p, lo, hi - lo + 1)
    assert np.array_equal(got[m - lo], bad[p][1][m - lo]) and not np.array_equal(got[m - lo], snap[p][1][m - lo])
    assert np.array_equal(got[hi - 1 - lo], snap[p][1][hi - 1 - lo])  # the independent gap resolved
    # ALL mode: the one walk cannot pass the record, nothing is written
    rows = e.reindex(all=True)
    assert e.last_reindex_rc == ECORRUPT and _counts(rows)[p][1:] == (0, 1)
    assert np.array_equal(e.read_index(p, lo, hi - lo + 1), got)


# ---- RMQ_REINDEX_ALL
@pytest.mark.parametrize("which", [1, 2])
def test_all_mode_on_clean_logs(state1, state2, which):
    e, cfg = state1 if which == 1 else state2
    rows, rc, after, snap, _, want = _damage_and_reindex(e, cfg, [], all_mode=True)
    assert rc == OK and not rows["entries_rewritten"].any() and not rows["gaps_unresolved"].any()
    assert [int(x) for x in rows["entries_live"]] == [want[p][1] for p in range(cfg.num_partitions)]
    assert sum(want[p][1] for p in want) > cfg.num_partitions
    U.assert_clean(after, e, cfg)


def test_all_mode_heals_damage(state1):
    e, cfg = state1
    changes = [c for p in (0, 5) for c in _two_gaps(e, cfg, p)]
    rows, rc, after, snap, _, _ = _damage_and_reindex(e, cfg, changes, all_mode=True)
    assert rc == OK and [_counts(rows)[p][1:] for p in (0, 5)] == [(2, 0)] * 2
    _assert_bytes(e, cfg, snap)


def test_all_mode_corrects_a_self_consistent_entry(fresh1):
    e, cfg = fresh1
    I = cfg.index_interval
    p = 2
    lo, hi = _live(e, cfg, p)
    ents = e.read_index(p, lo, hi - lo + 1)
    recs = U.host_walk(e, cfg, 0, p)[2]
    starts = {x[1]: i for i, x in enumerate(recs)}
    # an entry whose record is followed by another record start at or before the next entry
    for k in range(1, len(ents) - 1):
        i = starts.get(int(ents[k][1]))
        if i is not None and i + 1 < len(recs) and recs[i + 1][1] <= int(ents[k + 1][1]) and ents[k][1] > ents[k - 1][1]:
            break
    else:
        raise AssertionError("no such entry")
    m, (o, x), (o2, x2, _) = lo + k, (int(ents[k][0]), int(ents[k][1])), recs[i + 1]
    assert o2 == o + 1 and x2 > x
    changes = [(p, m, OFF, o ^ o2), (p, m, POS, x ^ x2)]  # the record start after the right one
    snap = R.snapshot(e, cfg)
    states, cons = e.states(), e.consumer_table()
    bad = _damaged(snap, I, changes)
    _damage(e, changes)
    assert e.read_index(p, m, 1).tolist() == [[o2, x2]]
    U.assert_clean(e.scrub(), e, cfg)  # the scrub passes it: containment and order hold
    rows = e.reindex()
    assert e.last_reindex_rc == OK and not rows["entries_rewritten"].any() and not rows["gaps_unresolved"].any()
    _assert_bytes(e, cfg, bad)
    want = X.model(bad, I, True)
    assert want[p][2:] == (1, 0)
    rows = e.reindex(all=True)
    assert e.last_reindex_rc == OK and _counts(rows) == {q: w[1:] for q, w in want.items()}
    assert int(rows["entries_rewritten"].sum()) == 1
    _assert_bytes(e, cfg, snap)
    assert np.array_equal(e.states(), states) and np.array_equal(e.consumer_table(), cons)


# ---- life goes on
def test_appends_and_fetches_after_a_rebuild(oracle_mod):
    cfg = U.cfg1()
    p = 3
    with Engine(cfg) as e, oracle_mod.OracleEngine(cfg) as o:
        ops = [("append", Batch(np.array([7], np.uint32), np.array([0], np.uint32), np.zeros(0, np.uint8)))]
        ops += [("append", Batch(*U.batch1(b))) for b in range(U.BATCHES1)]
        run_ops(e, o, cfg, ops, full_rings=True)
        st = e.state(p)
        first = st["log_start_offset"]
        one = np.array([p], np.uint32)
        # a read-then-commit consumer before the damage: it holds a cached position
        pre = [("consumer_commit", one, np.array([1], np.uint32), np.array([first + 2], np.uint64)),
               ("fetch", one, np.array([1]), np.array([5]), None, True)]
        run_ops(e, o, cfg, pre, full_rings=True)
        lo, hi = _live(e, cfg, p)
        # the entry the next batch's retention takes the log start from (FORMAT.md §4)
        per_batch = sum(16 + ((x + 15) & ~15) for x in U.LENS1)
        m_star = -(-(st["log_end_pos"] + per_batch - cfg.segment_bytes) // cfg.index_interval)
        assert lo + 1 < m_star < hi - 1
        ms = [lo, m_star, hi]
        snap = R.snapshot(e, cfg, [p])
        around = sorted({int(snap[p][1][m - lo][0]) + d for m in ms for d in (-1, 0, 1)})
        around = [t for t in around if first <= t < st["log_end_offset"]]
        _damage(e, [(p, ms[0], OFF, 1 << 1), (p, ms[1], POS, 1 << 40), (p, ms[2], POS, 1 << 2)])
        rows = e.reindex()
        assert e.last_reindex_rc == OK and _counts(rows)[p][1:] == (3, 0)
        post = [("fetch", one, np.array([1]), np.array([4]), None, True)]
        for t in around:  # fetches at the offsets around the rebuilt entries
            post += [("consumer_commit", one, np.array([2], np.uint32), np.array([t], np.uint64)),
                     ("fetch", one, np.array([2]), np.array([3]))]
        # further batches force retention through the rebuilt entries
        post += [("append", Batch(*U.batch1(b))) for b in range(U.BATCHES1, U.BATCHES1 + 2)]
        post += [("fetch", one, np.array([1]), np.array([6]), None, True), ("fetch", one, np.array([2]), np.array([6]))]
        run_ops(e, o, cfg, post, full_rings=True)
        assert e.state(p)["log_start_pos"] > snap[p][1][m_star - lo][1] > st["log_start_pos"]
        U.assert_clean(e.scrub(), e, cfg)


# ---- followers over a transport
def _heal_on_every_rank(engs, cfgs, views, r, damaged_rank, pick):
    """The collective call after rank `damaged_rank` damaged an entry of a partition it follows."""
    e, cfg, view = engs[r], cfgs[r], views[r]
    rf = cfg.replication_factor
    slots = lambda p: [s for s in range(rf) if view.ranks[p][s] == r]  # noqa: E731
    changes = []
    if r == damaged_rank:
        p = next(p for p in range(cfg.num_partitions) if pick(p, view))
        assert slots(p) and not e.state(p)["is_leader"]
        lo, hi = _live(e, cfg, p)
        assert hi - lo >= 2
        changes = [(p, (lo + hi) // 2, POS, 1 << 2)]
    rows, rc, scrub, snap, _, _ = _damage_and_reindex(e, cfg, changes, slots=slots, dry=False)  # collective
    assert rc == OK and int(rows["entries_rewritten"].sum()) == len(changes) and not rows["gaps_unresolved"].any()
    if changes:
        assert _counts(rows)[changes[0][0]][1] == 1
    _assert_bytes(e, cfg, snap)
    assert e.last_scrub_rc == OK and (scrub["status"] == OK).all()  # every rank's scrub is clean


def test_follower_after_truncation():
    # tests/repl_sim.py's leader-change script, as test_gpu_scrub.py runs it: rank 0 cuts its
    # divergent tail and follows its former partitions at term 2
    world, rf, ppr, group = 3, 3, 6, 2
    spec = StreamSpec(ppr, 300, "uniform", size=(0, 120), config_index=71)
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=1 << 16, index_interval=256,
                        max_batch_records=4096, max_batch_bytes=1 << 20, pipeline_depth=group)
    views, new, phases = leader_change_script(spec, world, rf, ppr, group)
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    hub = LocalHub(world)
    engs = [Engine(c) for c in cfgs]
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
            _heal_on_every_rank(engs, cfgs, final, r, 0, lambda p, view: p == 0)

        _run_ranks(world, body)
        assert engs[0].state(0)["term"] == 2 and not engs[0].state(0)["is_leader"]
    finally:
        for e in engs:
            e.close()
        hub.close()


def test_follower_after_rebase():
    # rank 0's regions are lost for 9 rounds, as test_gpu_scrub.py loses them: its followers fall
    # more than the ring behind and are rebased at the leader's rebase point
    world, rf, rounds = 3, 3, 12
    spec = StreamSpec(1, 10, "uniform", size=(100, 100), config_index=58)
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=1 << 13, index_interval=256,
                        max_batch_records=4096, max_batch_bytes=1 << 20, pipeline_depth=1)
    views = [rank_view(r, world, 1, rf) for r in range(world)]
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    hub = LocalHub(world)
    engs = [Engine(c) for c in cfgs]
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
            if r == 1:  # its copy of rank 0's partition restarted past its old end
                p = next(p for p in range(cfgs[r].num_partitions) if views[r].ranks[p][0] == 0)
                assert e.state(p)["log_start_offset"] > 0
            _heal_on_every_rank(engs, cfgs, views, r, 1, lambda p, view: view.ranks[p][0] == 0)

        _run_ranks(world, body)
    finally:
        for e in engs:
            e.close()
        hub.close()


# ---- refusals
def test_range_and_argument_errors(state1):
    e, cfg = state1
    P = cfg.num_partitions
    for first, n in ((0, P + 1), (P, 1), (P + 1, 0), (3, P - 2)):
        with pytest.raises(EngineError) as ei:
            e.reindex(first, n)
        assert ei.value.status == A.RMQ_ENOPART, (first, n)
    assert len(e.reindex(P, 0)) == 0 and len(e.reindex(0, 0)) == 0 and e.last_reindex_rc == OK
    for flags in (4, 7, 0x80000000):  # an unknown flag bit
        assert e.lib.rmq_reindex(e.h, 0, 1, flags, None) == A.RMQ_EINVAL
    assert e.lib.rmq_reindex(e.h, 0, P, 0, None) == OK  # res is nullable
    assert e.lib.rmq_fault_flip_index(e.h, 0, 0, 2, 1) == A.RMQ_EINVAL
    assert e.lib.rmq_fault_flip_index(e.h, 0, 0, 0, 0) == A.RMQ_EINVAL
    assert e.lib.rmq_fault_flip_index(e.h, P, 0, 0, 1) == A.RMQ_ENOPART
    U.assert_clean(e.scrub(), e, cfg)


def test_partition_without_a_local_replica():
    cfg = U.cfg1()
    with Engine(cfg) as e:
        U.fill1(e)
        e.set_replicas(6, [1, 2, 3], 0)  # the empty partition moves to other ranks: no local slot
        for mode in (False, True):
            rows = e.reindex(all=mode)
            assert e.last_reindex_rc == OK and int(rows[6]["replicas"]) == 0 and _counts(rows)[6] == (0, 0, 0)
            assert int(rows[5]["replicas"]) == 3 and _counts(rows)[5][0] > 0
