"""The model of rmq_fetch_bytes (tests/fetch_budget_util.py) on the oracle engine, without a GPU:
every sweep of tests/test_gpu_fetch_budget.py contains the categories it claims, so no GPU test can
pass by having nothing to trim; and the two exports load and refuse a null engine."""
import ctypes as C

import numpy as np
import pytest

import fetch_budget_util as B
import scrub_util as U
from ripplemq_amd import _abi as A


@pytest.fixture(scope="module")
def ora1(oracle_mod):
    e, cfg = B.filled1(oracle_mod.OracleEngine)
    yield e, cfg
    e.close()


@pytest.fixture(scope="module")
def ora3(oracle_mod):
    e, cfg = B.filled3(oracle_mod.OracleEngine)
    yield e, cfg
    e.close()


def test_symbols_load_and_refuse_a_null_engine():
    lib = A.load()
    assert {"rmq_fetch_bytes", "rmq_fetch_bytes_async"} <= set(A.header_symbols())
    used, t = C.c_uint64(7), C.c_uint64()
    assert lib.rmq_fetch_bytes(None, None, None, 1, A.RMQ_MEM_HOST, None, 0, None, C.byref(used)) == A.RMQ_EINVAL
    assert used.value == 0
    assert lib.rmq_fetch_bytes_async(None, None, None, 1, A.RMQ_MEM_HOST, None, 0, None, C.byref(t)) == A.RMQ_EINVAL


def test_sweep_on_state_1_has_every_category(ora1):
    ora, cfg = ora1
    sweep = B.sweep1(ora)
    cats = B.count_categories(sweep.values())
    print("state 1 sweep:", cats)
    assert sum(cats.values()) == len(B.SWEEP_MAX) * len(B.SWEEP_BUDGETS) * B.P1 * B.NC1
    assert all(cats[c] > 0 for c in B.CATEGORIES), cats
    for (mx, b), (rc, res, out, used, cat, _) in sweep.items():
        assert rc == A.RMQ_OK and used == int(res["bytes"].sum())
        served = res["status"] == A.RMQ_OK
        assert (res["bytes"][served] <= b).all()  # a served request never exceeds its budget
        z = np.array([c == "zero" for c in cat])
        assert (res["status"][z] == A.RMQ_ENOSPC).all() and (res["reserved"][z] > b).all()
        assert not res["reserved"][~z].any()


def test_eoffset_row_keeps_its_answer_whatever_the_budget(ora1):
    ora, cfg = ora1
    lo = ora.state(3)["log_start_offset"]
    assert lo > 0
    pidx, cons = B.all_reqs1()
    ora.commit_consumer_offset(np.array([3], np.uint32), np.array([1], np.uint32), np.array([lo - 1], np.uint64))
    try:
        for b in (0, 16, 512):
            res = B.model_fetch(ora, pidx, cons, 10, b)[1]
            r = res[3 * B.NC1 + 1]
            assert (int(r["status"]), int(r["start_offset"]), int(r["count"]), int(r["reserved"])) == (A.RMQ_EOFFSET, lo, 0, 0)
    finally:
        hi = ora.state(3)["log_end_offset"]
        ora.commit_consumer_offset(np.array([3], np.uint32), np.array([1], np.uint32),
                                   np.array([lo + (hi - lo) // 3], np.uint64))


def test_cut_point_edges_on_state_3_exist(ora3):
    ora, cfg = ora3
    calls, big, s = B.edge_calls3(ora, cfg)
    assert len(calls) == 6 + 18 and big.sum() >= 10
    I = cfg.index_interval
    assert int(s[1:B.NC3 + 1][big].max()) >= 16 * I  # a record spanning 16 intervals or more
    pidx, cons = np.full(B.NC3, B.P3), np.arange(B.NC3)
    cats = [B.model_fetch(ora, pidx, cons, 0xFFFFFFFF, b)[4] for b in calls]
    # s_j - 16 and s_j - 1: nothing fits; s_j and s_j + 1: one record; s_j + s_{j+1}: two, exactly
    for k, want in ((1, "zero"), (2, "one"), (3, "one"), (5, "boundary")):
        assert all(c == want for c in cats[k]), (k, set(cats[k]))
    assert set(cats[0]) == {"zero", "untrimmed"}  # (s_j = 16: the budget 0 is none)
    assert set(cats[4]) == {"one"}  # s_j + s_{j+1} - 16: cut to one record
    # the limit in every interval of the large records: never more than the first record is served
    sn = s[1:B.NC3 + 1][big]
    for i in range(18):
        c = np.array(cats[6 + i])[big]
        inside = 1024 * i < sn  # the limit falls inside the large record
        assert all(x == "one" for x in c[inside]), (i, c[inside])
        assert inside.any() == (i < 17)  # every interval of a record of up to 17 intervals is met
    assert all(x == "one" for x in np.array(cats[6 + 3])[big])  # 3 KiB in: inside every large record


def test_grid_and_chunk_edges_on_state_4_exist(oracle_mod):
    cfg = U.cfg4()
    with oracle_mod.OracleEngine(cfg) as ora:
        U.fill4(ora)
        for n in B.N4:
            pidx, cons, mx, bud = B.reqs4(n)
            rc, res, out, used, cats, _ = B.model_fetch(ora, pidx, cons, mx, bud)
            _, res0, _, used0 = ora.fetch(pidx, cons, mx)
            trimmed = np.array([c in ("zero", "one", "mid", "boundary") for c in cats])
            print(n, B.count_categories([(0, 0, 0, 0, cats)]))
            if n >= 15:
                assert trimmed.any()
            if n > 256:  # a trimmed request in the first chunk of 256 moves every later chunk
                assert trimmed[:256].any() and used < used0
                assert (res["out_pos"][256:] < res0["out_pos"][256:]).all()
            if n == 2500:
                assert all(trimmed[c * 256:(c + 1) * 256].any() for c in range(10))
