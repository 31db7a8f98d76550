"""The model of RMQ_FETCH_FILL (tests/fetch_fill_util.py) on the oracle engine, without a GPU: every
answer is bounded by out_cap, serves contiguous bytes from 0 and leaves the rows before the crossing
request as the unbounded call has them, and every sweep of tests/test_gpu_fetch_fill.py contains the
categories it claims, so no GPU test can pass by having nothing to cut or to put off."""
import numpy as np
import pytest

import fetch_budget_util as B
import fetch_fill_util as F
import scrub_util as U
from ripplemq_amd import _abi as A


@pytest.fixture(scope="module")
def ora1(oracle_mod):
    e, cfg = B.filled1(oracle_mod.OracleEngine)
    yield e, cfg
    e.close()


def test_sweep_on_state_1_has_every_category(ora1):
    ora, cfg = ora1
    sweep = F.sweep1(ora)
    for mx, (full, models) in sweep.items():
        cats = F.count_categories(models.values())
        print("state 1 sweep, max", mx, len(models), "capacities:", cats)
        assert sum(cats.values()) == len(models) * F.P1 * F.NC1
        # (max = 1: a slice of one record is served whole or not at all, so nothing is cut with k* >= 1)
        assert all(cats[c] > 0 for c in F.CATEGORIES if mx > 1 or c not in ("cut_mid", "cut_boundary")), (mx, cats)
        for cap, want in models.items():
            F.check_properties(want, full, cap)


def test_committing_model_moves_only_the_served(ora1, oracle_mod):
    """commit=True: the consumers of whole and cut rows move to start + count, pending ones stay."""
    ora, cfg = ora1
    o2, _ = B.filled1(oracle_mod.OracleEngine)
    try:
        pidx, cons = B.all_reqs1()
        full = F.unbounded(o2, pidx, cons, 10)
        cap = full[3] // 2 & ~15
        before = np.stack([o2.consumer_offsets(p) for p in range(F.P1)])
        rc, res, out, used, cats = F.model_fill(o2, pidx, cons, 10, None, cap, commit=True)
        F.check_properties((rc, res, out, used, cats), full, cap)
        after = np.stack([o2.consumer_offsets(p) for p in range(F.P1)])
        assert "pending" in cats and "whole" in cats
        for r, c in enumerate(cats):
            p, k = int(pidx[r]), int(cons[r])
            if c == "pending" or c.startswith("cut_zero"):
                assert after[p, k] == before[p, k]
            elif int(res["status"][r]) == A.RMQ_OK:
                assert after[p, k] == int(res["start_offset"][r]) + int(res["count"][r])
    finally:
        o2.close()


def test_cut_point_edges_on_state_3_exist(oracle_mod):
    ora, cfg = B.filled3(oracle_mod.OracleEngine)
    try:
        pidx, cons, two, full, j, caps = F.edge_calls3(ora, cfg)
        want = {0: "cut_zero_pending", 1: "cut_zero_pending", 2: "cut_boundary", 3: "cut_mid", 4: "cut_mid"}
        for k in range(6):
            cap = caps[k]
            m = F.model_fill(ora, pidx, cons, two, None, cap, full=full)
            F.check_properties(m, full, cap)
            assert m[4][j] == (want[k] if k in want else "whole"), (k, m[4][j])
            if k == 5:  # s_j + s_{j+1}: request j whole, the next one crosses with nothing
                assert m[4][j + 1] == "cut_zero_pending"
    finally:
        ora.close()


@pytest.mark.parametrize("budgets", [False, True])
def test_grid_and_chunk_edges_on_state_4_exist(oracle_mod, budgets):
    cfg = U.cfg4()
    with oracle_mod.OracleEngine(cfg) as ora:
        U.fill4(ora)
        for n in B.N4:
            hit = []
            for rstar, shift, cap, full in F.calls4(ora, n, budgets):
                pidx, cons, mx, bud = F.reqs4(n, shift, budgets)
                m = F.model_fill(ora, pidx, cons, mx, bud, cap, full=full)
                F.check_properties(m, full, cap)
                if rstar is None:
                    assert set(m[4]) == {"fits"}
                else:
                    assert m[4][rstar].startswith("cut"), (n, rstar, m[4][rstar])
                    hit.append(rstar)
            assert hit == F.targets4(n)
            if n == 2500:  # a cut in the first chunk puts every later chunk off whole
                assert hit == [0, 15, 16, 17, 255, 256, 257, 511, 512, 2499]
