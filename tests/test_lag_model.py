"""The model of rmq_lag (tests/lag_util.py) on the CPU: it agrees with the oracle's own fetch, its
headroom is the edge FORMAT.md §7 "Lag" says it is, and the request lists of tests/test_gpu_lag.py
hold every category they claim. No GPU."""
import numpy as np
import pytest

import lag_util as L
import scrub_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import LAG_RES_DTYPE, Engine
from ripplemq_amd.state_machine import PartitionBroker
from ripplemq_amd.tier import DurableLog

NONE = L.NONE


def test_python_entry_points_exist():
    assert LAG_RES_DTYPE.itemsize == 64 and LAG_RES_DTYPE.names[:3] == ("start_offset", "records", "bytes")
    assert callable(Engine.lag) and callable(Engine.lag_device)
    assert callable(PartitionBroker.consumer_lag) and callable(DurableLog.backlog)


def _agrees_with_fetch(ora, pidx, cons, offs, rows, scratch: int) -> int:
    """Every RMQ_OK row with records against the oracle's fetch from the same offset, committed to
    the scratch consumer, with max_records = 0xFFFFFFFF and an output sized to fit."""
    seen = 0
    for r in np.flatnonzero((rows["status"] == A.RMQ_OK) & (rows["records"] > 0)):
        p, off = int(pidx[r]), int(rows["start_offset"][r])
        ora.commit_consumer_offset([p], [scratch], [off])
        rc, res, _, used = ora.fetch([p], [scratch], [0xFFFFFFFF])
        assert rc == A.RMQ_OK and int(res["status"][0]) == A.RMQ_OK
        assert (int(res["start_offset"][0]), int(res["count"][0]), int(res["bytes"][0])) == \
            (off, int(rows["records"][r]), int(rows["bytes"][r])), (r, rows[r], res[0])
        assert used == int(rows["bytes"][r]) == int(rows["end_pos"][r]) - int(rows["start_pos"][r])
        seen += 1
    return seen


def test_model_agrees_with_the_oracles_fetch(oracle_mod):
    ora, cfg = L.filled1(oracle_mod.OracleEngine, max_consumers=5)
    with ora:
        pidx, cons, offs = L.sweep_reqs1(ora)
        rows = L.model_lag(ora, pidx, cons, offs)
        # (six active partitions, each retaining more than ten records)
        assert _agrees_with_fetch(ora, pidx, cons, offs, rows, scratch=4) > 6 * 10
    with oracle_mod.OracleEngine(U.cfg1(max_consumers=5)) as ora:
        L.scenario2(ora)
        st = ora.state(L.LAGGING2[0])
        assert st["log_start_offset"] < st["high_watermark"] < st["log_end_offset"]
        pidx, cons, offs = L.reqs2(ora)
        rows = L.model_lag(ora, pidx, cons, offs)
        assert _agrees_with_fetch(ora, pidx, cons, offs, rows, scratch=4) > 5
    with oracle_mod.OracleEngine(U.cfg3()) as ora:
        L.scenario3(ora)
        pidx, cons = L.reqs3()
        rows = L.model_lag(ora, pidx, cons)
        assert (rows["status"] == A.RMQ_OK).all() and (rows["records"] > 0).all()
        keep = np.arange(0, len(pidx), 7)  # (every seventh pair: each fetch copies a whole log)
        assert _agrees_with_fetch(ora, pidx[keep], cons[keep], None, rows[keep], scratch=0) == len(keep)


# ---- the headroom's edge on the oracle
def _random_state(oracle_mod, seed: int):
    """cfg1's shape; partition 0 takes 1 to 12 batches of 1 to 12 records of 0 to 600 B, so that
    retention has run in most states; a random retained record."""
    g = np.random.default_rng(seed)
    ora = oracle_mod.OracleEngine(U.cfg1())
    for _ in range(int(g.integers(1, 13))):
        lens = g.integers(0, 601, int(g.integers(1, 13))).astype(np.uint32)
        if int((16 + ((lens.astype(np.int64) + 15) & ~15)).sum()) > 4096 - 256:
            lens = lens[:4]
        ora.append(np.zeros(len(lens), np.uint32), lens, g.integers(0, 256, int(lens.sum()), dtype=np.uint8))
    st = ora.state(0)
    off = int(g.integers(st["log_start_offset"], st["high_watermark"]))
    return ora, st, off, g


def test_headroom_is_the_edge_on_the_oracle(oracle_mod):
    S, I = 4096, 256
    retained_states = evicting = survived = 0
    for seed in range(140):
        ora, st, off, g = _random_state(oracle_mod, seed)
        with ora:
            retained_states += st["log_start_offset"] > 0
            row = L.model_lag(ora, [0], [0], [off])[0]
            assert int(row["status"]) == A.RMQ_OK and int(row["start_offset"]) == off and int(row["records"]) > 0
            h = int(row["headroom"])
            assert h % 16 == 0 and 0 <= h <= S
            # exactly h bytes in several batches: the record survives
            nb = min(int(g.integers(2, 5)), h // 16)
            while nb:
                parts = L.split_bytes(h, nb, g)
                if max(sum(x) for x in parts) <= S - I:
                    break
                nb += 1
            for k, sizes in enumerate(parts if nb else []):
                _, s2 = ora.append(*L.bytes_batch(0, sizes, seed + k))
                assert s2["appended"] == len(sizes), s2
            after = ora.state(0)
            assert after["log_end_pos"] == st["log_end_pos"] + h
            assert after["log_start_offset"] <= off, (seed, h, st, after)
            survived += 1
        # a fresh copy of the state: one batch of h + 16 bytes evicts it
        if h + 16 > S - I:
            continue
        ora, st2, off2, _ = _random_state(oracle_mod, seed)
        with ora:
            assert (st2, off2) == (st, off)
            _, s2 = ora.append(*L.bytes_batch(0, [h + 16], seed))
            assert s2["appended"] == 1
            assert ora.state(0)["log_start_offset"] > off, (seed, h, st, ora.state(0))
            evicting += 1
    assert survived >= 100 and evicting >= 30 and retained_states >= 70, (survived, evicting, retained_states)


# ---- the request lists of the GPU file
def test_request_lists_hold_their_categories(oracle_mod):
    O = oracle_mod.OracleEngine
    lists = []
    ora, cfg = L.filled1(O)
    with ora:
        pidx, cons, offs = L.sweep_reqs1(ora)
        rows = L.model_lag(ora, pidx, cons, offs)
        lists.append(L.categorize(ora, pidx, cons, offs, rows))
        assert {"never_committed", "empty_partition"} <= set.union(*lists[-1])
        done = set()
        for pp, cc, oo in L.commit_rounds1(ora):
            ora.commit_consumer_offset(pp, cc, oo)
            done |= set(zip(pp.tolist(), cc.tolist()))
            rows = L.model_lag(ora, pp, cc)
            # a committed offset is answered as the same explicit one
            L.assert_rows(rows, L.model_lag(ora, pp, cc, oo))
            lists.append(L.categorize(ora, pp, cc, None, rows, committed=done))
    with O(U.cfg1()) as ora:
        L.scenario2(ora)
        a, b = (ora.state(p) for p in L.LAGGING2)
        assert a["log_start_offset"] < a["high_watermark"] < a["log_end_offset"]
        assert b["high_watermark"] == 0 < b["log_start_offset"]  # below the log start
        pidx, cons, offs = L.reqs2(ora)
        rows = L.model_lag(ora, pidx, cons, offs)
        lists.append(L.categorize(ora, pidx, cons, offs, rows))
        assert "hw_to_leo" in set.union(*lists[-1])
        assert not rows["records"][pidx == L.LAGGING2[1]].any()
    with O(U.cfg4()) as ora:
        L.scenario4(ora)
        pidx, cons, offs = L.reqs4()
        rows = L.model_lag(ora, pidx, cons, offs)
        cats = L.categorize(ora, pidx, cons, offs, rows)
        lists.append(cats)
        for n in L.N4:  # every n holds a served row; from 17 rows on, error rows among them
            assert (rows["status"][:n] == A.RMQ_OK).any()
            if n > L.WG:
                assert {"enopart", "einval", "enotleader"} <= set.union(*cats[:n]), n
    with O(U.cfg1()) as ora:
        cur = L.scenario6(ora)
        p = np.array(list(cur), np.uint32)
        rows = L.model_lag(ora, p, np.zeros(len(p)), replica=True, cursor=cur)
        assert (rows["status"] == A.RMQ_EOFFSET).any() and (rows["records"] > 0).sum() >= 3
        plain = L.model_lag(ora, [L.FOLLOWED1], [0])
        assert int(plain["status"][0]) == A.RMQ_ENOTLEADER
    count = L.count_categories(lists)
    assert all(count[c] > 0 for c in L.CATEGORIES), count


def test_high_base_scenario_has_retained_and_evicted_rows(oracle_mod):
    cfg = L.H.cfg_high()
    with oracle_mod.OracleEngine(cfg) as ora:
        L.H.rebase_oracle(ora, L.high_bases(cfg.index_interval))
        for b in L.H.scenario_batches(5, config_index=75):
            ora.append(b.pidx, b.lens, b.payload)
        pidx, cons, offs = L.reqs5(ora)
        rows = L.model_lag(ora, pidx, cons, offs)
        for p in (0, L.HIGH_P):
            mine = rows[pidx == p]
            # (three explicit offsets below the log start, and the consumer that never moved)
            assert (mine["status"] == A.RMQ_EOFFSET).sum() == 4 and (mine["records"] > 0).sum() > 10
        bases = L.high_bases(cfg.index_interval)
        up = L.shift_rows(rows, pidx, bases)
        moved = up[pidx == L.HIGH_P]
        assert (moved["start_offset"] > 2 ** 32).all() and (moved["start_pos"][moved["records"] > 0] > 2 ** 40).all()
        for f in ("records", "bytes", "evicted", "headroom", "status"):
            assert np.array_equal(up[f], rows[f])


@pytest.mark.parametrize("total,batches", [(16, 1), (32, 2), (4096, 4), (160, 3)])
def test_split_bytes(total, batches):
    g = np.random.default_rng(total)
    for _ in range(20):
        parts = L.split_bytes(total, batches, g)
        assert len(parts) == batches and sum(map(sum, parts)) == total
        assert all(s >= 16 and s % 16 == 0 for x in parts for s in x)
