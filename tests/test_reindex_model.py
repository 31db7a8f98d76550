"""The host model of rmq_reindex (tests/reindex_util.py) on the CPU oracle: the entries it rebuilds
from a clean log by the definition of FORMAT.md §5 (the first record start at or after m * I, the
log end counting as one) equal the entries the oracle's appends wrote, on the states of
tests/scrub_util.py and on the edge shapes of the live range; and what the model makes of damaged
entries in default and ALL mode."""
import numpy as np
import pytest

import reindex_util as X
import repair_util as R
import scrub_util as U


def _check_all(e, cfg):
    """Every partition's rebuilt entries equal read_index; returns the snapshot."""
    I = cfg.index_interval
    snap = R.snapshot(e, cfg)
    for p, (st, ents, rs) in snap.items():
        got = X.rebuild(st, rs, I)
        lo, hi = X.live_range(st, I)
        assert got is not None and got.shape == (max(hi - lo + 1, 0), 2), p
        assert np.array_equal(got, ents.reshape(-1, 2)), (p, got, ents)
    for mode in (False, True):
        for p, (new, live, rw, unres) in X.model(snap, I, mode).items():
            lo, hi = X.live_range(snap[p][0], I)
            assert (live, rw, unres) == (max(hi - lo + 1, 0), 0, 0) and np.array_equal(new, snap[p][1].reshape(-1, 2))
    return snap


@pytest.fixture(scope="module")
def snap1(oracle_mod):
    cfg = U.cfg1()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill1(e)
        yield _check_all(e, cfg), cfg


def test_state1(snap1):
    snap, cfg = snap1
    I = cfg.index_interval
    # records over 2 and 6 intervals: runs of equal consecutive entries; rings wrapped
    st, ents, _ = snap[0]
    assert st["log_end_pos"] > cfg.segment_bytes and st["log_start_pos"] > 0
    assert any(np.array_equal(a, b) for a, b in zip(ents, ents[1:]))
    # partition 6 is an empty log on a multiple: its one live entry is the log start
    st6, e6, _ = snap[6]
    assert (st6["log_start_pos"], st6["log_end_pos"]) == (0, 0) and e6.tolist() == [[0, 0]]
    assert X.live_range(snap[7][0], I) == (0, 0)


def test_state2(oracle_mod):
    cfg = U.cfg2()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill2(e)
        snap = _check_all(e, cfg)
    assert any(st["log_end_pos"] > cfg.segment_bytes for st, _, _ in snap.values())


def test_state3(oracle_mod):
    cfg = U.cfg3()
    with oracle_mod.OracleEngine(cfg) as e:
        U.fill3(e)
        _check_all(e, cfg)


def _fill_multiples(e, batches):
    """Records of exactly one interval (240 payload bytes at I = 256) on partition 0."""
    for _ in range(batches):
        _, st = e.append(np.zeros(8, np.uint32), np.full(8, 240, np.uint32), np.arange(8 * 240, dtype=np.uint8))
        assert st["appended"] == 8, st


def test_log_start_on_a_multiple(oracle_mod):
    cfg = U.cfg1()
    with oracle_mod.OracleEngine(cfg) as e:
        _fill_multiples(e, 3)
        snap = _check_all(e, cfg)
    st, ents, _ = snap[0]
    I = cfg.index_interval
    assert st["log_start_pos"] > 0 and st["log_start_pos"] % I == 0
    assert ents[0].tolist() == [st["log_start_offset"], st["log_start_pos"]]  # E[lo] is the log start itself


def test_no_live_entry():
    """A log between two multiples has no live entry (appends alone cannot leave one on a single
    engine: a rebased follower's can be), so this state is made by hand: one segment, one walk."""
    cfg = U.cfg1()
    ring = np.zeros(cfg.segment_bytes, np.uint8)
    ring[16:24] = np.frombuffer((5).to_bytes(8, "little"), np.uint8)  # offset 5, length 0, crc 0
    st = dict(log_start_pos=16, log_end_pos=32, log_start_offset=5, log_end_offset=6, segment_bytes=cfg.segment_bytes)
    assert X.rebuild(st, {0: ring}, cfg.index_interval).shape == (0, 2)
    for mode in (False, True):
        new, live, rw, unres = X.model_part(st, np.zeros((0, 2), np.uint64), {0: ring}, cfg.index_interval, mode)
        assert (len(new), live, rw, unres) == (0, 0, 0, 0)
    ring[28] ^= 1  # its crc: the one segment fails, and its walk cannot land
    assert X.model_part(st, np.zeros((0, 2), np.uint64), {0: ring}, cfg.index_interval)[1:] == (0, 0, 1)


@pytest.mark.parametrize("where", ["lo", "mid", "hi"])
@pytest.mark.parametrize("word,mask", [(0, 1 << 3), (1, 1 << 2), (1, 1 << 40)])
def test_single_flips_heal(snap1, where, word, mask):
    snap, cfg = snap1
    I = cfg.index_interval
    p = 2
    lo, hi = X.live_range(snap[p][0], I)
    m = {"lo": lo, "mid": (lo + hi) // 2, "hi": hi}[where]
    bad = X.with_entries(snap, I, p, [(m, word, mask)])
    new, live, rw, unres = X.model_part(*bad[p], I)
    assert (live, rw, unres) == (hi - lo + 1, 1, 0) and np.array_equal(new, snap[p][1])
    assert X.model_part(*bad[p], I, True)[1:] == (hi - lo + 1, 1, 0)


def test_record_damage_on_every_slot_is_unresolved_and_one_slot_is_not(snap1):
    snap, cfg = snap1
    I, S = cfg.index_interval, cfg.segment_bytes
    p = 1
    st, ents, rs = snap[p]
    lo, hi = X.live_range(st, I)
    m = lo + 3
    bad = X.with_entries(snap, I, p, [(m, 0, 1)])
    pos = int(ents[m - lo - 1][1])  # the record the gap's walk starts on
    one = R.apply_flips(bad, [(0, p, (pos + 12) % S, 0x5A)])
    new, _, rw, unres = X.model_part(*one[p], I)
    assert (rw, unres) == (1, 0) and np.array_equal(new, ents)
    every = R.apply_flips(bad, [(r, p, (pos + 12) % S, 0x5A) for r in range(3)])
    new, _, rw, unres = X.model_part(*every[p], I)
    assert (rw, unres) == (0, 1) and np.array_equal(new, bad[p][1])
    assert X.model_part(*every[p], I, True)[2:] == (0, 1)
    # the repair's model leaves the index-damaged partition unrepaired, healed or not by rmq_reindex
    assert R.model({p: one[p]}, I)[1][p][2] > 0
