"""The host model of rmq_repair_remote (tests/repair_remote_util.py) on per-rank CPU oracles driven
through repl_sim's rounds and commit notices, at the shape of tests/test_gpu_repair_remote.py. Every
damage scenario of that file is applied to numpy copies of the snapshots: the model restores the
pre-damage rings exactly where it claims a fetch and leaves every other byte alone."""
import numpy as np
import pytest

import repair_remote_util as M
import repair_util as R
from repl_sim import exchange_round, notice_round, place, rank_cfg
from ripplemq_amd.sharding import rank_view


def _world(oracle_mod, world, drop=(), big=()):
    views = [rank_view(r, world, M.PPR, 3) for r in range(world)]
    cfgs = [rank_cfg(M.base_cfg(3), views[r], r) for r in range(world)]
    oras = [oracle_mod.OracleEngine(c) for c in cfgs]
    try:
        for r in range(world):
            place(oras[r], views[r], world)
            if r in big:
                n = cfgs[r].num_partitions
                oras[r].set_segments(np.arange(n, dtype=np.uint32), np.full(n, 2 * M.SEG, np.uint64))
        for k in range(M.BATCHES):
            for r in range(world):
                _, st = oras[r].append(*M.batch(r, k))
                assert st["appended"] == len(M.batch(r, k)[0]), (r, k, st)
            exchange_round(oras, drop=drop if k == M.BATCHES - 1 else ())
            notice_round(oras)
        return [M.snapshot(oras[r], cfgs[r], views[r], r) for r in range(world)]
    finally:
        for o in oras:
            o.close()


@pytest.fixture(scope="module")
def snaps3(oracle_mod):
    return _world(oracle_mod, 3)


def _rings(s):
    return {p: rs for p, (_, _, rs) in s.parts.items()}


def _same(a, b):
    return all(np.array_equal(a[p][sl], b[p][sl]) for p in b for sl in b[p])


def _run(clean, flips, **kw):
    bad = [M.apply_flips(s, flips.get(r, [])) for r, s in enumerate(clean)]
    return bad, M.model(bad, M.INTERVAL, **kw)


def test_the_shape_reaches_every_path(snaps3):
    for s in snaps3:
        for p, (st, ents, rs) in s.parts.items():
            assert len(rs) == 1 and st["commit"] == st["log_end_offset"]  # one slot per rank, all committed
            assert st["log_start_pos"] > 0 and st["log_end_pos"] > M.SEG  # retention moved the start; the log wrapped
            segs = R.segments(st, ents, M.INTERVAL)
            assert None not in segs and any(a == b for a, b, _, _ in segs)  # some segments are empty
            if s.key[p] == 0:  # the partition the scenarios damage: one segment wraps the ring end
                assert any(a < b and a % M.SEG > (b - 1) % M.SEG for a, b, _, _ in segs)
            assert any(x[2] > 1024 for x in M.records(s, p, M.slot_of(s, p)))
    # committed logs are byte-identical across the ranks that hold them
    for gp in range(3 * M.PPR):
        logs = []
        for s in snaps3:
            p = M.local_of(s, gp)
            st, _, rs = s.parts[p]
            logs.append((st["log_start_pos"], st["log_end_pos"], R.seg_bytes(rs[M.slot_of(s, p)], st["log_start_pos"], st["log_end_pos"])))
        assert all(x[:2] == logs[0][:2] and np.array_equal(x[2], logs[0][2]) for x in logs)
    res = M.model(snaps3, M.INTERVAL)
    assert all(r.served == (0, 0) and not r.statuses and all(c == (0, 0, 0, 0, 0) for c in r.rows.values()) for r in res)


@pytest.mark.parametrize("what", M.CLASSES + ("big",))
@pytest.mark.parametrize("rank", [1, 0])
def test_one_damaged_rank_is_served_by_its_first_candidate(snaps3, what, rank):
    s = snaps3[rank]
    p = M.local_of(s, 0)
    sl = M.slot_of(s, p)
    flip, si, seg = M.flip_of(s, p, sl, what)
    bad, res = _run(snaps3, {rank: [flip]})
    assert not R.passes(bad[rank].parts[p][2][sl], seg) and R.passes(s.parts[p][2][sl], seg)
    donor = M.candidates(s, p)[0]
    assert donor == (0 if rank else s.ranks[p][1])
    nb = seg[1] - seg[0]
    assert res[rank].rows[p] == (0, 0, 1, nb, 0) and res[rank].statuses == [(0, donor, p, sl, si, M.SERVED)]
    assert [r.served for r in res] == [(1, nb) if q == donor else (0, 0) for q in range(3)]
    assert all(_same(res[q].rings, _rings(snaps3[q])) for q in range(3))
    # a dry run counts the same and writes nothing
    _, dry = _run(snaps3, {rank: [flip]}, dry=True)
    assert dry[rank].rows == res[rank].rows and [r.served for r in dry] == [r.served for r in res]
    assert all(_same(dry[q].rings, _rings(bad[q])) for q in range(3))


def _same_segment(snaps, seg, ranks):
    out = {}
    for r in ranks:
        p = M.local_of(snaps[r], 0)
        out[r] = [M.same_segment_flip(snaps[r], p, M.slot_of(snaps[r], p), seg)]
    return out


def test_damaged_first_donor_and_damage_everywhere(snaps3):
    p0 = M.local_of(snaps3[0], 0)
    flip0, si, seg = M.flip_of(snaps3[0], p0, 0, "payload")
    f, third = snaps3[0].ranks[p0][1], snaps3[0].ranks[p0][2]
    flips = {0: [flip0], **_same_segment(snaps3, seg, [f])}
    bad, res = _run(snaps3, flips)
    assert [s[-1] for s in res[0].statuses] == [s[-1] for s in res[f].statuses] == [M.BADWALK, M.SERVED]
    assert res[third].served == (2, 2 * (seg[1] - seg[0])) and res[0].served == res[f].served == (0, 0)
    assert all(_same(res[q].rings, _rings(snaps3[q])) for q in range(3))
    flips = {0: [flip0], **_same_segment(snaps3, seg, [1, 2])}
    bad, res = _run(snaps3, flips)
    for q in range(3):
        assert _same(res[q].rings, _rings(bad[q])) and res[q].served == (0, 0)  # no byte changes anywhere
        assert res[q].rows[flips[q][0][1]] == (0, 0, 0, 0, 1)
        assert [s[-1] for s in res[q].statuses] == [M.BADWALK, M.BADWALK]


@pytest.mark.parametrize("second_damaged", [False, True])
def test_response_corrupted_in_flight(snaps3, second_damaged):
    s = snaps3[1]
    p = M.local_of(s, 0)
    sl = M.slot_of(s, p)
    flip, si, seg = M.flip_of(s, p, sl, "payload")
    second = M.candidates(s, p)[1]
    flips, ranges = {1: [flip]}, None
    if second_damaged:
        flips.update(_same_segment(snaps3, seg, [second]))
        ranges = [None if r != second else [] for r in range(3)]
    bad, res = _run(snaps3, flips, corrupt=[(0, 1, -5)], ranges=ranges)
    if second_damaged:
        assert [x[-1] for x in res[1].statuses] == [M.SERVED, M.BADWALK] and res[1].rows[p] == (0, 0, 0, 0, 1)
        assert all(_same(res[q].rings, _rings(bad[q])) for q in range(3))  # the refused span left nothing behind
    else:
        assert [x[-1] for x in res[1].statuses] == [M.SERVED, M.SERVED] and res[1].rows[p][2] == 1
        assert res[0].served == res[second].served == (1, seg[1] - seg[0])
        assert all(_same(res[q].rings, _rings(snaps3[q])) for q in range(3))


def test_uncommitted_tail_is_never_asked_for(oracle_mod):
    snaps = _world(oracle_mod, 3, drop=(0,))
    st = snaps[0].parts[0][0]
    assert st["commit"] < st["log_end_offset"]
    flip, si, seg = M.flip_of(snaps[0], 0, 0, "crc", below=st["log_end_offset"], above=st["commit"])
    assert seg[3] > st["commit"]
    bad, res = _run(snaps, {0: [flip]})
    assert res[0].statuses == [] and res[0].rows[0] == (0, 0, 0, 0, 1)
    assert all(r.served == (0, 0) for r in res) and all(_same(res[q].rings, _rings(bad[q])) for q in range(3))


def test_ring_sizes_and_log_starts_differ(oracle_mod):
    snaps = _world(oracle_mod, 3, big=(1, 2))
    p0, p1 = M.local_of(snaps[0], 0), M.local_of(snaps[1], 0)
    sl1 = M.slot_of(snaps[1], p1)
    st0, st1 = snaps[0].parts[p0][0], snaps[1].parts[p1][0]
    assert (st0["segment_bytes"], st1["segment_bytes"]) == (M.SEG, 2 * M.SEG)
    assert st1["log_start_offset"] < st0["log_start_offset"] and st1["log_end_pos"] == st0["log_end_pos"]
    flip_a, si_a, seg_a = M.flip_of(snaps[1], p1, sl1, "payload", below=st0["log_start_offset"] - 8)
    flip_b, si_b, seg_b = M.flip_of(snaps[0], p0, 0, "payload")
    assert seg_a[1] <= st0["log_start_pos"] and seg_b[0] % M.SEG != seg_b[0] % (2 * M.SEG)
    bad, res = _run(snaps, {0: [flip_b], 1: [flip_a]})
    second = M.candidates(snaps[1], p1)[1]
    assert res[1].statuses == [(0, 0, p1, sl1, si_a, M.OUTSIDE), (1, second, p1, sl1, si_a, M.SERVED)]
    assert res[0].statuses == [(0, M.candidates(snaps[0], p0)[0], p0, 0, si_b, M.SERVED)]
    assert all(_same(res[q].rings, _rings(snaps[q])) for q in range(3))


@pytest.mark.parametrize("both", [False, True])
def test_two_local_slots(oracle_mod, both):
    snaps = _world(oracle_mod, 2)
    s = snaps[1]
    p = M.local_of(s, 0)
    assert sorted(s.parts[p][2]) == [1, 2]
    flip, si, seg = M.flip_of(s, p, 2, "payload")
    flips = [flip] + ([M.same_segment_flip(s, p, 1, seg)] if both else [])
    bad, res = _run(snaps, {1: flips})
    nb = seg[1] - seg[0]
    assert res[1].rows[p] == ((0, 0, 2, 2 * nb, 0) if both else (1, nb, 0, 0, 0))
    assert res[0].served == ((2, 2 * nb) if both else (0, 0))
    assert all(_same(res[q].rings, _rings(snaps[q])) for q in range(2))


def test_ranges_select_what_is_repaired_not_who_serves(snaps3):
    s = snaps3[1]
    p = M.local_of(s, 0)
    flip, si, seg = M.flip_of(s, p, M.slot_of(s, p), "crc")
    bad, res = _run(snaps3, {1: [flip]}, ranges=[[], [p], None])
    assert res[0].rows == {} and res[0].served == (1, seg[1] - seg[0]) and list(res[1].rows) == [p]
    assert all(_same(res[q].rings, _rings(snaps3[q])) for q in range(3))
    other = next(q for q in s.parts if q != p)
    bad, res = _run(snaps3, {1: [flip]}, ranges=[None, [other], None])  # the damaged partition is outside the range
    assert res[1].rows[other] == (0, 0, 0, 0, 0) and _same(res[1].rings, _rings(bad[1])) and res[0].served == (0, 0)
