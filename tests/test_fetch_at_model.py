"""The model of rmq_fetch_at (tests/fetch_at_util.py) on the oracle engine, without a GPU: the sweep
of tests/test_gpu_fetch_at.py contains every category it claims, so no GPU test can pass by having
nothing to address; the model leaves the oracle as it found it; and the two exports are in the
header and the binding table, load, and refuse a null engine."""
import ctypes as C

import numpy as np
import pytest

import fetch_at_util as F
from ripplemq_amd import _abi as A


@pytest.fixture(scope="module")
def ora1(oracle_mod):
    e, cfg = F.filled1(oracle_mod.OracleEngine)
    yield e, cfg
    e.close()


def test_symbols_load_and_refuse_a_null_engine():
    lib = A.load()
    assert {"rmq_fetch_at", "rmq_fetch_at_async"} <= set(A.header_symbols())
    assert {"rmq_fetch_at", "rmq_fetch_at_async"} <= set(A._SIGS)
    used, t = C.c_uint64(7), C.c_uint64()
    assert lib.rmq_fetch_at(None, None, None, None, 1, A.RMQ_MEM_HOST, None, 0, None, C.byref(used)) == A.RMQ_EINVAL
    assert used.value == 0
    assert lib.rmq_fetch_at_async(None, None, None, None, 1, A.RMQ_MEM_HOST, None, 0, None, C.byref(t)) == A.RMQ_EINVAL


def test_sweep_on_state_1_has_every_category(ora1):
    ora, cfg = ora1
    before = F.tables(ora)
    sweep = F.sweep1(ora)
    cats = F.count_categories(sweep)
    print("state 1 sweep:", cats)
    assert sum(cats.values()) == len(F.SWEEP_MAX) * F.N_SWEEP
    assert all(cats[c] > 0 for c in F.CATEGORIES), cats
    assert np.array_equal(F.tables(ora), before)  # the model put every row back
    pidx, cons, offs = F.sweep_reqs1(ora)
    for mx, ((rc, res, out, used), cat) in sweep.items():
        assert rc == A.RMQ_OK and used == int(res["bytes"].sum())
        ex = offs != np.uint64(F.NONE)
        ok = ex & (res["status"] == A.RMQ_OK)
        assert (res["start_offset"][ok] == offs[ok]).all()  # served or empty: the slice starts where asked
        # the requests without an offset answer as the plain fetch of their own consumer does
        _, plain, _, _ = ora.fetch(pidx, cons, np.full(len(pidx), mx))
        for f in ("start_offset", "count", "bytes", "status"):
            assert np.array_equal(res[f][~ex], plain[f][~ex]), f


def test_offsets_past_the_high_watermark_and_2_32_are_empty_and_ok(ora1):
    ora, cfg = ora1
    hw = ora.state(3)["high_watermark"]
    offs = np.array([hw, hw + 1, 2 ** 32 + 5, 2 ** 53 + 1, 2 ** 64 - 2], np.uint64)
    for mx in F.SWEEP_MAX:
        rc, res, out, used = F.model_fetch_at(ora, np.full(5, 3), np.zeros(5), mx, offs)
        assert (rc, used) == (A.RMQ_OK, 0) and not res["status"].any() and not res["count"].any()
        assert np.array_equal(res["start_offset"], offs)


def test_commit_is_a_seek_and_a_read(ora1):
    ora, cfg = ora1
    before = F.tables(ora)
    try:
        lo = ora.state(2)["log_start_offset"]
        pidx, cons = np.array([2, 3, 4]), np.array([1, 1, 1])
        offs = np.array([lo + 3, ora.state(3)["log_start_offset"] - 1, F.NONE], np.uint64)
        rc, res, out, used = F.model_fetch_at(ora, pidx, cons, 5, offs, commit=True)
        assert [int(x) for x in res["status"]] == [A.RMQ_OK, A.RMQ_EOFFSET, A.RMQ_OK]
        after = F.tables(ora)
        assert int(after[2, 1]) == lo + 3 + 5
        assert int(after[3, 1]) == ora.state(3)["log_start_offset"]
        assert int(after[4, 1]) == int(before[4, 1]) + int(res["count"][2])
        after[[2, 3, 4], 1] = before[[2, 3, 4], 1]
        assert np.array_equal(after, before)  # nothing else moved, the scratch rows included
    finally:
        ora.commit_consumer_offset(np.array([2, 3, 4], np.uint32), np.ones(3, np.uint32), before[[2, 3, 4], 1])


def test_grid_edges_on_state_4_mix_all_three_kinds(oracle_mod):
    import fetch_budget_util as B
    import scrub_util as U
    with oracle_mod.OracleEngine(F.cfg4()) as ora:
        U.fill4(ora)
        for n in B.N4:
            pidx, cons, mx, offs = F.reqs4(n)
            rc, res, out, used = F.model_fetch_at(ora, pidx, cons, mx, offs)
            assert rc == A.RMQ_OK
            if n >= 16:  # a partially filled last workgroup holds served requests of both explicit kinds
                served = res["count"] > 0
                assert (served & (offs == 0)).any() and (served & (offs == 1)).any()
                assert (res["start_offset"][served & (offs == 1)] == 1).all()
