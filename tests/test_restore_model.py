"""The host model of rmq_restore (tests/restore_util.py) pinned to the CPU oracle: seeded scenarios
run until rings have wrapped and retention has run, every partition's exact retained window is taken
from the oracle's ring and fed to the model, and the model's state, window bytes and live index
entries must equal the oracle's own (repair_util.snapshot). Also the shapes the GPU tests rely on,
and the damage classes against the model's verdicts."""
import numpy as np
import pytest

import repair_util as R
import restore_util as M
from ripplemq_amd import _abi as A


def _scenario(oracle_mod, cfg, batches):
    with oracle_mod.OracleEngine(cfg) as o:
        M.fill(o, batches)
        snap = R.snapshot(o, cfg)
        wins = {p: M.window(o, cfg, p) for p in range(cfg.num_partitions)}
    return snap, wins


@pytest.fixture(scope="module")
def main(oracle_mod):
    cfg = M.cfg_main()
    return (cfg,) + _scenario(oracle_mod, cfg, M.batches_main())


@pytest.fixture(scope="module")
def big(oracle_mod):
    cfg = M.cfg_big()
    return (cfg,) + _scenario(oracle_mod, cfg, M.batches_big())


def _check(cfg, snap, wins):
    S, I, RF = cfg.segment_bytes, cfg.index_interval, cfg.replication_factor
    for p, (run, tab, it) in wins.items():
        st, ents, rings = snap[p]
        m = M.model(run, tab, it, S, I, range(RF), RF)
        n = st["log_end_offset"] - st["log_start_offset"]
        assert m["row"] == (A.RMQ_OK, n, run.size, M.NONE, 0), (p, m["row"])
        for f in M.STATE_FIELDS:
            assert m["state"][f] == st[f], (p, f, m["state"][f], st[f])
        assert m["state"]["leader_commit"] == st["leader_commit"]
        at = np.arange(st["log_start_pos"], st["log_end_pos"]) % S
        for r in range(RF):
            assert np.array_equal(m["rings"][r][at], rings[r][at]), (p, r)
        assert np.array_equal(m["index"][1], ents), (p, m["index"], ents)
        assert not M.host_refuses(run, tab, it)


def test_model_equals_the_oracle_main(main):
    _check(*main)


def test_model_equals_the_oracle_big(big):
    _check(*big)


def test_main_scenario_reaches_every_shape(main):
    cfg, snap, wins = main
    S, I = cfg.segment_bytes, cfg.index_interval
    st = {p: snap[p][0] for p in snap}
    wraps = [p for p in st if st[p]["log_start_pos"] % S > (st[p]["log_end_pos"] - 1) % S and st[p]["log_end_pos"] > st[p]["log_start_pos"]]
    assert 0 in wraps or 1 in wraps, "a window wraps the ring end"
    assert st[0]["log_start_offset"] > 0 and st[1]["log_start_offset"] > 0, "retention has run"
    assert st[2]["log_end_pos"] - st[2]["log_start_pos"] == S and st[2]["log_start_pos"] % I == 0 and st[2]["log_start_pos"]
    assert any(st[p]["log_start_pos"] % I for p in (0, 1)), "a first_pos that is no multiple of I"
    assert (st[3]["log_end_offset"], st[3]["log_end_pos"]) == (1, 16), "a 16-byte record with an empty payload, alone"
    assert st[4]["log_end_offset"] - st[4]["log_start_offset"] == 1 and st[4]["log_start_offset"] == 1
    assert [st[p]["log_end_offset"] - st[p]["log_start_offset"] for p in (5, 6, 7)] == [64, 65, 129]
    # a record over three intervals: equal consecutive index entries
    assert any((np.diff(snap[p][1][:, 1].astype(np.int64)) == 0).sum() >= 2 for p in (0, 1))
    lens = {x[2] for p in (0, 1) for x in M.record_map(wins[p][1], wins[p][0], wins[p][2])}
    assert {0, 15, 16, 17, 100, 241, 600} <= lens  # what the flip classes pick
    recs0 = M.record_map(wins[0][1], wins[0][0], wins[0][2])
    assert any((x[1] % S) + 16 + x[2] > S for x in recs0), "a record straddles the ring end in partition 0"


def test_big_scenario_takes_the_whole_wave_path(big):
    cfg, snap, wins = big
    for p in range(4):
        recs = M.record_map(wins[p][1], wins[p][0], wins[p][2])
        assert recs[-1][2] > 9000 and any(x[2] <= 1024 for x in recs) and any(x[2] > 1024 for x in recs)
    st = snap[0][0]
    assert st["log_start_offset"] > 0 and st["log_end_pos"] > cfg.segment_bytes


@pytest.mark.parametrize("what", R.CLASSES1 + M.TABLE_CLASSES)
def test_damage_classes(main, what):
    cfg, snap, wins = main
    S, I, RF = cfg.segment_bytes, cfg.index_interval, cfg.replication_factor
    p = 0 if what == "straddle" else 1
    run, tab, it = wins[p]
    brun, btab = M.class_damage(run, tab, it, S, what)
    assert (brun != run).sum() + (btab != tab).sum() == 1
    assert M.host_refuses(brun, btab, it)
    row = M.model(brun, btab, it, S, I, range(RF), RF)["row"]
    fo, n = int(it["first_offset"][0]), int(it["count"][0])
    assert row[0] == A.RMQ_ECORRUPT and fo <= row[3] < fo + n and row[4] in (M.CRC, M.CHAIN)
    want = {"payload": M.CRC, "padding": M.CRC, "crc": M.CRC, "offset": M.CHAIN, "len_top": M.CHAIN,
            "straddle": M.CRC, "table_word": M.CHAIN, "table_last": M.CHAIN, "table_zero": M.CHAIN}
    if what in want:
        assert row[4] == want[what], (what, row)
    if what == "table_zero":
        assert row[3] == fo
    if what == "table_last":
        assert row[3] == fo + n - 1
    if what in R.CLASSES1:  # a damaged record is reported where the host walk stops
        from ripplemq_amd.tier import _scan
        assert row[3] == fo + _scan(brun, fo, n, True, False)[0]
