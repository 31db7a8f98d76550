"""The host model of rmq_repair (tests/repair_util.py) on the CPU oracle: states 1 and 2 of
tests/scrub_util.py, every damage scenario of tests/test_gpu_repair.py applied to numpy copies of
the rings. The flips land where each scenario says, the model's output rings equal the clean rings
wherever a donor exists, and the host walk accepts the whole repaired log."""
import numpy as np
import pytest

import repair_util as R
import scrub_util as U


@pytest.fixture(scope="module")
def snap1(oracle_mod):
    cfg = U.cfg1()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill1(e)
        recs = {p: U.host_walk(e, cfg, 0, p)[2] for p in range(cfg.num_partitions)}
        yield R.snapshot(e, cfg), recs, cfg


@pytest.fixture(scope="module")
def snap2(oracle_mod):
    cfg = U.cfg2()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill2(e)
        recs = {p: U.host_walk(e, cfg, 0, p)[2] for p in range(cfg.num_partitions)}
        yield R.snapshot(e, cfg), recs, cfg


def _same(a, b):
    return all(np.array_equal(a[p][r], b[p][r]) for p in a for r in a[p])


def _clean_rings(snap):
    return {p: rs for p, (_, _, rs) in snap.items()}


@pytest.mark.parametrize("which", [1, 2])
def test_clean_states_need_nothing(snap1, snap2, which):
    snap, _, cfg = snap1 if which == 1 else snap2
    rings, counts = R.model(snap, cfg.index_interval)
    assert all(c == (0, 0, 0) for c in counts.values()), counts
    assert _same(rings, _clean_rings(snap))
    for p, (st, ents, rs) in snap.items():
        segs = R.segments(st, ents, cfg.index_interval)
        assert None not in segs and segs[0][0] == st["log_start_pos"] and segs[-1][1] == st["log_end_pos"]
        assert all(a[1] == b[0] and a[3] == b[2] for a, b in zip(segs, segs[1:]))  # the segments tile the log
        assert all(np.array_equal(rs[0], rs[r]) for r in rs)  # (FORMAT.md §2: byte-identical slots)


def _one_class(snap, recs, cfg, what, p):
    S, I = cfg.segment_bytes, cfg.index_interval
    st, ents, _ = snap[p]
    rec, flip = R.class_flip(recs[p], S, what, p)
    segs = R.segments(st, ents, I)
    s = R.seg_of(segs, rec[1])
    bad = R.apply_flips(snap, [flip])
    # the flip lies inside the record's bytes, in its segment, on the class slot only
    d = (flip[2] - rec[1]) % S
    assert d < 16 + ((rec[2] + 15) & ~15) and segs[s][0] <= rec[1] + d < segs[s][1]
    assert [R.passes(bad[p][2][r], segs[s]) for r in range(3)] == [True, True, False]
    assert not R.log_ok(bad[p][2][R.CLASS_SLOT], st)
    rings, counts = R.model(bad, I)
    want = {q: (0, 0, 0) for q in snap}
    want[p] = (1, segs[s][1] - segs[s][0], 0)
    assert counts == want
    assert _same(rings, _clean_rings(snap))
    assert all(R.log_ok(rings[p][r], st) for r in range(3))
    return segs[s], rec


@pytest.mark.parametrize("what", R.CLASSES1)
def test_one_flip_per_class(snap1, what):
    snap, recs, cfg = snap1
    seg, rec = _one_class(snap, recs, cfg, what, R.class_partition(what))
    S = cfg.segment_bytes
    if what == "straddle":  # the segment wraps the ring end
        assert seg[0] % S > (seg[1] - 1) % S


def test_big_tail(snap2):
    snap, recs, cfg = snap2
    p = next(p for p in range(4) if any(x[2] == 5000 for x in recs[p]))
    seg, _ = _one_class(snap, recs, cfg, "big_tail", p)
    assert seg[1] - seg[0] > cfg.index_interval  # longer than one interval: several 1 KiB steps of the copy


@pytest.mark.parametrize("which", ["distinct", "same", "all3"])
def test_several_pairs(snap1, which):
    snap, recs, cfg = snap1
    I = cfg.index_interval
    st, ents, _ = snap[R.MULTI_P]
    segs = R.segments(st, ents, I)
    flips = R.multi_flips(recs[R.MULTI_P], recs[R.OTHER_P], segs, cfg.segment_bytes, which)
    bad = R.apply_flips(snap, flips)
    rings, counts = R.model(bad, I)
    hit = {}  # segment -> slots damaged in it
    for slot, p, off, _ in flips:
        if p == R.MULTI_P:
            pos = next(x[1] for x in recs[p] if (x[1] + 12) % cfg.segment_bytes == off)
            hit.setdefault(R.seg_of(segs, pos), set()).add(slot)
    assert counts[R.OTHER_P][0] == 1 and counts[R.OTHER_P][2] == 0
    assert np.array_equal(rings[R.OTHER_P][1], snap[R.OTHER_P][2][1])
    if which == "distinct":
        assert len(hit) == 2 and counts[R.MULTI_P][0] == 2 and counts[R.MULTI_P][2] == 0
    elif which == "same":
        assert list(hit.values()) == [{0, 1}] and counts[R.MULTI_P][0] == 2 and counts[R.MULTI_P][2] == 0
    else:
        assert list(hit.values()) == [{0, 1, 2}] and counts[R.MULTI_P] == (0, 0, 3)
        assert all(np.array_equal(rings[R.MULTI_P][r], bad[R.MULTI_P][2][r]) for r in range(3))  # every byte unchanged
        return
    assert _same(rings, _clean_rings(snap))
    assert all(R.log_ok(rings[R.MULTI_P][r], st) for r in range(3))


def test_outside_the_log(snap1):
    snap, _, cfg = snap1
    st = snap[7][0]
    assert (st["log_end_offset"], st["log_start_pos"], st["log_end_pos"]) == (1, 0, 16)
    bad = R.apply_flips(snap, [(2, 7, 16, 0x5A), (2, 7, 100, 0x5A)])
    rings, counts = R.model(bad, cfg.index_interval)
    assert counts[7] == (0, 0, 0)
    assert np.array_equal(rings[7][2], bad[7][2][2]) and not np.array_equal(rings[7][2], snap[7][2][2])
