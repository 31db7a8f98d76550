"""rmq_repair_remote on the GPU (FORMAT.md §10, "Remote repair") over the LocalHub on one device:
follower and leader damage, a damaged first donor, damage everywhere, an uncommitted tail, a response
corrupted in flight, two slots on one rank, the dry run, per-rank ranges and the call without a
transport. Every expected ring, counter and served pair comes from the host model
(tests/repair_remote_util.py, checked on the CPU by tests/test_repair_remote_model.py) over bytes read
back before the damage, never from the call under test."""
import numpy as np
import pytest

import repair_remote_util as M
import repair_util as R
import scrub_util as U
from repl_sim import place, rank_cfg
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine, LocalHub
from ripplemq_amd.sharding import rank_view
from test_gpu_scrub import _run_ranks

pytestmark = pytest.mark.gpu

OK, ECORRUPT = A.RMQ_OK, A.RMQ_ECORRUPT
ROW = ["bad_offset", "bad_replica", "bad_kind", "replicas", "status"]
COUNT = ["segments_repaired", "bytes_repaired", "segments_fetched", "bytes_fetched", "segments_unrepaired"]


class World:
    """`world` engines on one device behind a LocalHub, placed by rank_view and filled with
    M.BATCHES rounds (drop: ranks whose last round reaches no follower; big: ranks whose rings are
    doubled before the fill), synced."""

    def __init__(self, world, rf=3, drop=(), big=()):
        self.world, self.rf = world, rf
        self.views = [rank_view(r, world, M.PPR, rf) for r in range(world)]
        # (a doubled ring is allocated before the old one is released: room for both)
        self.cfgs = [rank_cfg(M.base_cfg(rf, pool_bytes=4 * M.SEG * len(self.views[r].gp) if r in big else 0),
                              self.views[r], r) for r in range(world)]
        self.hub = LocalHub(world)
        self.engs = [Engine(c) for c in self.cfgs]

        def fill(r):
            e = self.engs[r]
            e.attach_local(self.hub)
            place(e, self.views[r])
            if r in big:
                n = self.cfgs[r].num_partitions
                e.set_segments(np.arange(n, dtype=np.uint32), np.full(n, 2 * M.SEG, np.uint64))
            for k in range(M.BATCHES):
                if k == M.BATCHES - 1 and r in drop:
                    e.fault_drop_rounds(1)
                e.append_async(*M.batch(r, k))
                e.sync()
            e.sync()  # every follower's commit is what its leader committed

        try:
            self.run(fill)
        except BaseException:
            self.close()
            raise

    def run(self, body):
        out = [None] * self.world

        def wrap(r):
            out[r] = body(r)

        _run_ranks(self.world, wrap)
        return out

    def snaps(self):
        return self.run(lambda r: M.snapshot(self.engs[r], self.cfgs[r], self.views[r], r))

    def close(self):
        for e in self.engs:
            e.close()
        self.hub.close()


@pytest.fixture(scope="module")
def world3():
    w = World(3)
    yield w
    w.close()


def _counts(rows, first=0):
    return {first + i: tuple(int(r[f]) for f in COUNT) for i, r in enumerate(rows)}


def _rings(e, snap):
    return {p: {sl: e.read_segment(sl, p, 0, a.size) for sl, a in rs.items()} for p, (_, _, rs) in snap.parts.items()}


def _same_rings(got, want, what):
    for p, rs in want.items():
        for sl, a in rs.items():
            assert np.array_equal(got[p][sl], a), (what, p, sl, np.flatnonzero(got[p][sl] != a)[:8])


def _play(w, flips, ranges=None, dry=False, corrupt=(), old_limit=False, undo=True, peer_bytes=M.PEER_BYTES):
    """Snapshot every rank, model the damaged world, damage the engines, make the collective call,
    scrub, read everything back; the checks every scenario shares. flips: {rank: [(slot, p, ring
    offset, mask)]}; ranges: per rank (first, n) or None. Returns (clean snapshots, the model's
    results, per rank (rows, rc, served, the following scrub's rows, its rc, the old limit's rows))."""
    clean = w.snaps()
    bad = [M.apply_flips(s, flips.get(r, [])) for r, s in enumerate(clean)]
    rng = [None if ranges is None or ranges[r] is None else range(ranges[r][0], ranges[r][0] + ranges[r][1])
           for r in range(w.world)]
    want = M.model(bad, M.INTERVAL, ranges=rng, dry=dry, corrupt=corrupt, peer_bytes=peer_bytes)
    tables = w.run(lambda r: w.engs[r].consumer_table())

    def body(r):
        e = w.engs[r]
        for f in flips.get(r, []):
            e.fault_flip_ring(*f)
        for src, dst, at in corrupt:
            if src == r:
                e.fault_corrupt_repair(dst, at)
        old = e.repair(dry_run=True) if old_limit else None  # (collective: every rank makes it)
        first, n = (0, None) if ranges is None or ranges[r] is None else ranges[r]
        rows = e.repair_remote(first, n, dry_run=dry)
        rc, served = e.last_repair_rc, e.last_repair_served
        scrub = e.scrub()
        return rows, rc, served, scrub, e.last_scrub_rc, old

    got = w.run(body)
    after = w.snaps()
    for r in range(w.world):
        rows, rc, served, scrub, src, _ = got[r]
        first = 0 if ranges is None or ranges[r] is None else ranges[r][0]
        assert _counts(rows, first) == want[r].rows, (r, _counts(rows, first), want[r].rows)
        assert served == want[r].served, (r, served, want[r].served)
        _same_rings({p: rs for p, (_, _, rs) in after[r].parts.items()}, want[r].rings, ("model", r))
        # states and index entries stay, and so do the consumer tables
        for p, (st, ents, _) in clean[r].parts.items():
            assert after[r].parts[p][0] == st and np.array_equal(after[r].parts[p][1], ents), (r, p)
        full = ranges is None or ranges[r] is None
        if full:  # the rows are the following scrub's, or (dry run) the present state's
            assert rc == src and all(np.array_equal(rows[f], scrub[f]) for f in ROW), (r, rows, scrub)
    assert all(np.array_equal(a, b) for a, b in zip(tables, w.run(lambda r: w.engs[r].consumer_table())))
    if undo:  # leave the shared world clean: flip back whatever is still damaged
        def heal(r):
            e = w.engs[r]
            for sl, p, off, mask in flips.get(r, []):
                if e.read_segment(sl, p, off, 1)[0] != clean[r].parts[p][2][sl][off]:
                    e.fault_flip_ring(sl, p, off, mask)
            _same_rings(_rings(e, clean[r]), {p: rs for p, (_, _, rs) in clean[r].parts.items()}, ("undo", r))

        w.run(heal)
    return clean, want, got


def _clean_rings(snap):
    return {p: rs for p, (_, _, rs) in snap.parts.items()}


def _assert_healed(clean, want, ranks=None):
    """The model (and so, by _play, the engine) left every ring of these ranks byte-identical to
    what was read back before the damage."""
    for r in (range(len(clean)) if ranks is None else ranks):
        _same_rings(want[r].rings, _clean_rings(clean[r]), ("healed", r))


def _follower_flip(clean, rank, gp, what):
    s = clean[rank]
    p = M.local_of(s, gp)
    return p, M.flip_of(s, p, M.slot_of(s, p), what)


# ---- 1. follower damage (and 9: its dry run)
@pytest.mark.parametrize("what", M.CLASSES + ("big",))
def test_follower_damage_is_fetched_from_the_leader(world3, what):
    w = world3
    p, (flip, si, seg) = _follower_flip(w.snaps(), 1, 0, what)  # rank 1's slot of a partition rank 0 leads
    nb = seg[1] - seg[0]
    if what == "wrapped":
        assert seg[0] % M.SEG > (seg[1] - 1) % M.SEG
    clean, want, got = _play(w, {1: [flip]}, old_limit=True)
    old = got[1][5]
    assert int(old["segments_unrepaired"].sum()) == 1 and int(old[p]["segments_unrepaired"]) == 1  # the old limit
    assert all(not got[r][5]["segments_unrepaired"].any() for r in (0, 2))
    assert _counts(got[1][0])[p] == (0, 0, 1, nb, 0)
    assert [got[r][2] for r in range(3)] == [(1, nb), (0, 0), (0, 0)]
    assert all(got[r][1] == OK and got[r][4] == OK for r in range(3))
    assert want[1].statuses == [(0, 0, p, flip[0], si, M.SERVED)]
    _assert_healed(clean, want)


def test_dry_run_counts_and_writes_nothing(world3):
    w = world3
    p, (flip, si, seg) = _follower_flip(w.snaps(), 1, 0, "payload")
    nb = seg[1] - seg[0]
    clean, want, got = _play(w, {1: [flip]}, dry=True)
    assert _counts(got[1][0])[p] == (0, 0, 1, nb, 0) and got[0][2] == (1, nb)  # the real call's counters
    assert got[1][1] == ECORRUPT and int(got[1][0][p]["status"]) == ECORRUPT  # the present state
    bad = M.apply_flips(clean[1], [flip])
    _same_rings(want[1].rings, _clean_rings(bad), "dry")  # (so _play saw the damaged bytes unchanged)
    _assert_healed(clean, want, ranks=(0, 2))


# ---- 2. leader damage
@pytest.mark.parametrize("what", M.CLASSES)
def test_leader_damage_is_fetched_from_the_lowest_other_slot(world3, what):
    w = world3
    snaps = w.snaps()
    p = M.local_of(snaps[0], 0)
    flip, si, seg = M.flip_of(snaps[0], p, 0, what)
    donor = snaps[0].ranks[p][1]
    clean, want, got = _play(w, {0: [flip]})
    nb = seg[1] - seg[0]
    assert _counts(got[0][0])[p] == (0, 0, 1, nb, 0) and got[donor][2] == (1, nb)
    assert want[0].statuses == [(0, donor, p, 0, si, M.SERVED)]
    assert all(got[r][1] == OK for r in range(3))
    _assert_healed(clean, want)


# ---- 3. the first donor is damaged too
def test_damaged_first_donors_refuse_and_the_third_rank_serves(world3):
    w = world3
    snaps = w.snaps()
    p0 = M.local_of(snaps[0], 0)
    f = snaps[0].ranks[p0][1]  # the follower the leader asks first
    third = snaps[0].ranks[p0][2]
    flip0, si, seg = M.flip_of(snaps[0], p0, 0, "payload")
    pf = M.local_of(snaps[f], 0)
    flipf = M.same_segment_flip(snaps[f], pf, M.slot_of(snaps[f], pf), seg)
    clean, want, got = _play(w, {0: [flip0], f: [flipf]})
    nb = seg[1] - seg[0]
    assert want[0].statuses == [(0, f, p0, 0, si, M.BADWALK), (1, third, p0, 0, si, M.SERVED)]
    assert want[f].statuses == [(0, 0, pf, flipf[0], si, M.BADWALK), (1, third, pf, flipf[0], si, M.SERVED)]
    assert got[third][2] == (2, 2 * nb) and got[0][2] == got[f][2] == (0, 0)
    assert _counts(got[0][0])[p0] == _counts(got[f][0])[pf] == (0, 0, 1, nb, 0)
    assert all(got[r][1] == OK and got[r][4] == OK for r in range(3))
    _assert_healed(clean, want)


# ---- 4. the same segment damaged on all three ranks
def test_damage_on_every_rank_changes_nothing(world3):
    w = world3
    snaps = w.snaps()
    p0 = M.local_of(snaps[0], 0)
    flip0, si, seg = M.flip_of(snaps[0], p0, 0, "crc")
    flips = {0: [flip0]}
    for r in (1, 2):
        p = M.local_of(snaps[r], 0)
        flips[r] = [M.same_segment_flip(snaps[r], p, M.slot_of(snaps[r], p), seg)]
    clean, want, got = _play(w, flips)
    for r in range(3):
        p = flips[r][0][1]
        assert _counts(got[r][0])[p] == (0, 0, 0, 0, 1) and got[r][1] == ECORRUPT and got[r][2] == (0, 0)
        _same_rings(want[r].rings, _clean_rings(M.apply_flips(clean[r], flips[r])), ("all3", r))  # no byte changed
        assert [s[-1] for s in want[r].statuses] == [M.BADWALK, M.BADWALK]


# ---- 5. an uncommitted tail is never fetched
def test_uncommitted_tail_is_not_requested():
    w = World(3, drop=(0,))
    try:
        snaps = w.snaps()
        p = 0
        st = snaps[0].parts[p][0]
        assert st["commit"] < st["log_end_offset"]  # the dropped round's records are above the commit
        flip, si, seg = M.flip_of(snaps[0], p, 0, "crc", below=st["log_end_offset"], above=st["commit"])
        assert seg[3] > st["commit"]
        clean, want, got = _play(w, {0: [flip]}, undo=False)
        assert want[0].statuses == [] and _counts(got[0][0])[p] == (0, 0, 0, 0, 1) and got[0][1] == ECORRUPT
        assert got[1][2] == got[2][2] == (0, 0)
        _same_rings(want[0].rings, _clean_rings(M.apply_flips(clean[0], [flip])), "tail")
    finally:
        w.close()


# ---- 6. a response corrupted in flight
@pytest.mark.parametrize("second_damaged", [False, True])
def test_corrupted_response_writes_nothing(world3, second_damaged):
    w = world3
    snaps = w.snaps()
    p, (flip, si, seg) = _follower_flip(snaps, 1, 0, "payload")
    second = M.candidates(snaps[1], p)[1]
    flips, ranges = {1: [flip]}, None
    if second_damaged:
        # the ring between the rounds: nothing of the refused response may stay. The second candidate
        # holds the same damage and calls with n = 0, so it serves (status 3) and repairs nothing
        p2 = M.local_of(snaps[second], 0)
        flips[second] = [M.same_segment_flip(snaps[second], p2, M.slot_of(snaps[second], p2), seg)]
        ranges = [None if r != second else (0, 0) for r in range(3)]
    clean, want, got = _play(w, flips, ranges=ranges, corrupt=[(0, 1, -5)])
    nb = seg[1] - seg[0]
    assert got[0][2] == (1, nb)  # rank 0 served a span that passed at home
    if second_damaged:
        assert [s[-1] for s in want[1].statuses] == [M.SERVED, M.BADWALK]
        assert _counts(got[1][0])[p] == (0, 0, 0, 0, 1) and got[1][1] == ECORRUPT
        _same_rings(want[1].rings, _clean_rings(M.apply_flips(clean[1], flips[1])), "untouched")
        _assert_healed(clean, want, ranks=(0,))
    else:
        assert [s[-1] for s in want[1].statuses] == [M.SERVED, M.SERVED] and got[second][2] == (1, nb)
        assert _counts(got[1][0])[p] == (0, 0, 1, nb, 0) and got[1][1] == OK
        _assert_healed(clean, want)


# ---- 7. different ring sizes and log starts
def test_ring_sizes_and_log_starts_differ():
    """Both followers of rank 0's partitions keep 16 KiB rings, the leader 8 KiB: the followers retain
    records the leader has evicted. (With one doubled follower no other rank would hold such a span,
    so it could be refused but never served.)"""
    w = World(3, big=(1, 2))
    try:
        snaps = w.snaps()
        p0, p1 = M.local_of(snaps[0], 0), M.local_of(snaps[1], 0)
        sl1 = M.slot_of(snaps[1], p1)
        st0, st1 = snaps[0].parts[p0][0], snaps[1].parts[p1][0]
        assert (st0["segment_bytes"], st1["segment_bytes"]) == (M.SEG, 2 * M.SEG)
        assert st1["log_start_offset"] < st0["log_start_offset"] and st1["log_end_pos"] == st0["log_end_pos"]
        # A: rank 1, a segment below the leader's log start; B: the leader, a recent segment
        flip_a, si_a, seg_a = M.flip_of(snaps[1], p1, sl1, "payload", below=st0["log_start_offset"] - 8)
        flip_b, si_b, seg_b = M.flip_of(snaps[0], p0, 0, "payload")
        assert seg_a[1] <= st0["log_start_pos"] and seg_b[0] >= st0["log_start_pos"]
        assert seg_b[0] % M.SEG != seg_b[0] % (2 * M.SEG)  # the two sides store B at different ring offsets
        # C: rank 1 leads partition 2 on 16 KiB rings; its first candidate, rank 0, follows on 8 KiB
        pc, p0c = M.local_of(snaps[1], 2), M.local_of(snaps[0], 2)
        assert M.candidates(snaps[1], pc)[0] == 0 and snaps[0].parts[p0c][0]["segment_bytes"] == M.SEG
        flip_c, si_c, seg_c = M.flip_of(snaps[1], pc, 0, "crc", above=snaps[0].parts[p0c][0]["log_start_offset"] + 8)
        clean, want, got = _play(w, {0: [flip_b], 1: [flip_a, flip_c]}, undo=False)
        second = M.candidates(snaps[1], p1)[1]
        assert sorted(want[1].statuses) == sorted([(0, 0, p1, sl1, si_a, M.OUTSIDE), (1, second, p1, sl1, si_a, M.SERVED),
                                                   (0, 0, pc, 0, si_c, M.SERVED)])
        first0 = M.candidates(snaps[0], p0)[0]
        assert want[0].statuses == [(0, first0, p0, 0, si_b, M.SERVED)]
        assert _counts(got[1][0])[p1] == (0, 0, 1, seg_a[1] - seg_a[0], 0)
        assert _counts(got[1][0])[pc] == (0, 0, 1, seg_c[1] - seg_c[0], 0)
        assert _counts(got[0][0])[p0] == (0, 0, 1, seg_b[1] - seg_b[0], 0)
        assert all(got[r][1] == OK and got[r][4] == OK for r in range(3))
        _assert_healed(clean, want)
    finally:
        w.close()


# ---- 8. world 2, RF 3: one rank holds two slots of a partition
@pytest.mark.parametrize("both", [False, True])
def test_two_local_slots(both):
    w = World(2)
    try:
        snaps = w.snaps()
        p = M.local_of(snaps[1], 0)
        assert sorted(snaps[1].parts[p][2]) == [1, 2]
        flip, si, seg = M.flip_of(snaps[1], p, 2, "payload")
        flips = [flip] + ([M.same_segment_flip(snaps[1], p, 1, seg)] if both else [])
        clean, want, got = _play(w, {1: flips}, undo=False)
        nb = seg[1] - seg[0]
        if both:  # two requests to rank 0
            assert _counts(got[1][0])[p] == (0, 0, 2, 2 * nb, 0) and got[0][2] == (2, 2 * nb)
            assert [s[-1] for s in want[1].statuses] == [M.SERVED, M.SERVED]
        else:  # repaired locally, nothing asked
            assert _counts(got[1][0])[p] == (1, nb, 0, 0, 0) and got[0][2] == (0, 0) and want[1].statuses == []
        assert all(got[r][1] == OK and got[r][4] == OK for r in range(2))
        _assert_healed(clean, want)
    finally:
        w.close()


# ---- the per-destination budget
def test_a_pair_over_the_budget_waits(monkeypatch):
    monkeypatch.setenv("RMQ_REPAIR_PEER_BYTES", "48")  # (read at rmq_create) below any segment of the pair's class
    w = World(3)
    try:
        p, (flip, si, seg) = _follower_flip(w.snaps(), 1, 0, "big")
        assert seg[1] - seg[0] > 48
        clean, want, got = _play(w, {1: [flip]}, undo=False, peer_bytes=48)
        assert want[1].statuses == [] and _counts(got[1][0])[p] == (0, 0, 0, 0, 1) and got[1][1] == ECORRUPT
        assert all(got[r][2] == (0, 0) for r in range(3))
        _same_rings(want[1].rings, _clean_rings(M.apply_flips(clean[1], [flip])), "budget")
    finally:
        w.close()


# ---- 10. ranges, arguments, no transport
def test_ranges_are_local_and_a_rank_with_no_range_still_serves(world3):
    w = world3
    p, (flip, si, seg) = _follower_flip(w.snaps(), 1, 0, "crc")
    clean, want, got = _play(w, {1: [flip]}, ranges=[(0, 0), (p, 1), None])
    nb = seg[1] - seg[0]
    assert len(got[0][0]) == 0 and got[0][2] == (1, nb) and got[0][1] == OK
    assert len(got[1][0]) == 1 and _counts(got[1][0], p)[p] == (0, 0, 1, nb, 0) and got[1][1] == OK
    _assert_healed(clean, want)


def test_without_a_transport_it_is_rmq_repair():
    cfg = U.cfg1()
    with Engine(cfg) as e:
        U.fill1(e)
        P = cfg.num_partitions
        for flags in (2, 3, 0x80000000):  # an unknown flag bit
            assert e.lib.rmq_repair_remote(e.h, 0, 1, flags, None, None) == A.RMQ_EINVAL
        assert e.lib.rmq_repair_remote(e.h, 0, P + 1, 0, None, None) == A.RMQ_ENOPART
        assert e.lib.rmq_repair_remote(e.h, 0, P, 0, None, None) == OK and len(e.repair_remote(P, 0)) == 0
        for what in ("payload", "crc", "len_top", "straddle"):
            p = R.class_partition(what)
            recs = U.host_walk(e, cfg, R.CLASS_SLOT, p)[2]
            _, flip = R.class_flip(recs, cfg.segment_bytes, what, p)
            clean = R.snapshot(e, cfg)
            for dry in (True, False):
                e.fault_flip_ring(*flip)
                a = e.repair(dry_run=dry)
                rca = e.last_repair_rc
                if not dry:
                    e.fault_flip_ring(*flip)
                b = e.repair_remote(dry_run=dry)
                assert e.last_repair_rc == rca and e.last_repair_served == (0, 0)
                assert all(np.array_equal(a[f], b[f]) for f in a.dtype.names), (what, dry, a, b)
                assert not b["segments_fetched"].any() and not b["bytes_fetched"].any()
                if dry:
                    e.fault_flip_ring(*flip)  # (back to clean)
                else:
                    assert int(b[p]["segments_repaired"]) == 1
                for q, (_, _, rs) in clean.items():
                    for sl, ring in rs.items():
                        assert np.array_equal(e.read_segment(sl, q, 0, ring.size), ring), (what, dry, q, sl)
        e.profile(1)
        e.repair_remote()
        n, ms = e.profile_query(6)
        assert n == 1 and ms > 0 and e.profile_query(5)[0] == 0
