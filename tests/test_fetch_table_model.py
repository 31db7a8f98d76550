"""The model of rmq_fetch_table (tests/fetch_table_util.py) without a GPU: each sweep of
tests/test_gpu_fetch_table.py holds what it claims (owning rows and rows of every non-owning kind,
the counts at the lane and window edges, a record of more than 64 pieces inside a walked run, an
empty-payload record), the model's table agrees with parse_records, and table_records splits an
output exactly as parse_records does."""
import numpy as np
import pytest

import fetch_at_util as FA
import fetch_budget_util as B
import fetch_fill_util as F
import fetch_table_util as T
import scrub_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import parse_records, table_records


@pytest.fixture(scope="module")
def ora1(oracle_mod):
    e, cfg = FA.filled1(oracle_mod.OracleEngine)  # (state 1, with room for the explicit requests' scratch ids)
    yield e, cfg
    e.close()


@pytest.fixture(scope="module")
def ora3(oracle_mod):
    cfg = U.cfg3()
    e = oracle_mod.OracleEngine(cfg)
    U.fill3(e)
    yield e, cfg
    e.close()


def _agrees_with_parse_records(want):
    res, out = want[1], want[2]
    rec_row, rec_pos = T.table_of(res, out)
    split = table_records(out, res, rec_row, rec_pos)
    assert len(split) == len(res)
    for r in range(len(res)):
        lo, nb = int(res["out_pos"][r]), int(res["bytes"][r])
        if T.kind_of(res, r) != "owning":
            assert split[r] == [] and rec_row[r + 1] == rec_row[r]
            continue
        recs = parse_records(out[lo:lo + nb])
        assert split[r] == recs and len(recs) == int(res["count"][r])
        words = rec_pos[int(rec_row[r]):int(rec_row[r + 1])]
        assert words[0] == 0 and words[-1] == nb and len(words) == len(recs) + 1
        sizes = np.array([16 + ((len(b) + 15) & ~15) for _, _, b in recs])
        assert np.array_equal(np.diff(words.astype(np.int64)), sizes)
        assert np.array_equal(words, T.reference_walk(out[lo:lo + nb], len(recs)))


def _kinds(res):
    return {T.kind_of(res, r) for r in range(len(res))}


def test_state_1_holds_owning_empty_and_eoffset_rows(ora1):
    ora, cfg = ora1
    seen = set()
    for mx in B.SWEEP_MAX:
        want = T.plain1(ora, mx)
        seen |= _kinds(want[1])
        _agrees_with_parse_records(want)
        sizes = [len(b) for r in range(len(want[1])) if T.kind_of(want[1], r) == "owning"
                 for _, _, b in parse_records(want[2][int(want[1]["out_pos"][r]):][:int(want[1]["bytes"][r])])]
        assert 0 in sizes  # an empty-payload record (16 bytes) inside a walked run
    assert {"owning", "empty"} <= seen and "eoffset" not in seen
    # (the four committed offsets of state 1 all lie inside the retained logs: the RMQ_EOFFSET rows
    # come from fetch_at_util's sweep of explicit offsets, which the GPU test runs beside them)
    for mx in B.SWEEP_MAX:
        want = T.explicit1(ora, mx)[1]
        seen |= _kinds(want[1])
        _agrees_with_parse_records(want)
    assert {"owning", "empty", "eoffset"} <= seen


def test_budgets_and_fill_hold_both_enospc_kinds_and_pending_rows(ora1):
    ora, cfg = ora1
    pidx, cons = B.all_reqs1()
    seen = set()
    for b in B.SWEEP_BUDGETS:
        want = B.model_fetch(ora, pidx, cons, 1024, b)
        seen |= _kinds(want[1])
        _agrees_with_parse_records(want)
    assert "enospc_budget" in seen
    full = F.unbounded(ora, pidx, cons, 1024)
    small = B.model_fetch(ora, pidx, cons, 1024, 0, out_cap=(full[3] // 2) & ~15)  # no fill: the rest does not fit
    assert small[0] == A.RMQ_ENOSPC and "enospc_capacity" in _kinds(small[1])
    _agrees_with_parse_records(small)
    cats = set()
    for cap in T.fill_caps(full):
        want = F.model_fill(ora, pidx, cons, 1024, None, cap, full=full)
        cats |= set(want[4])
        seen |= _kinds(want[1])
        _agrees_with_parse_records(want)
    assert "pending" in seen and any(c.startswith("cut_") and not c.startswith("cut_zero") for c in cats)
    assert any(c.startswith("cut_zero") for c in cats)


def test_state_3_holds_the_edge_counts_and_big_records(ora3):
    ora, cfg = ora3
    counts, first_big, last_big, inner_big, pieces = set(), 0, 0, 0, set()
    for variant in ("start", "big_first", "big_last"):
        _, want = T.model3(ora, cfg, variant)
        res, out = want[1], want[2]
        assert want[0] == A.RMQ_OK and (res["status"] == A.RMQ_OK).all() and (res["count"] > 0).all()
        _agrees_with_parse_records(want)
        for r in range(len(res)):
            counts.add(int(res["count"][r]))
            lens = [len(b) for _, _, b in parse_records(out[int(res["out_pos"][r]):][:int(res["bytes"][r])])]
            first_big += lens[0] >= 1023 and variant == "big_first"
            last_big += lens[-1] >= 1023 and variant == "big_last"
            inner_big += any(x > 1024 for x in lens[1:-1])  # more than 64 pieces, inside the run
            assert max(lens) <= 16384
            if variant == "start":
                pieces |= {1 + (x + 15) // 16 for x in lens[:-1]}  # record sizes the walk steps over
    assert set(T.EDGE_COUNTS) <= counts, sorted(counts)
    assert {1, 2, 64, 65, 66, 1025} <= pieces  # from the empty payload to records of 65 to 1025 pieces
    assert first_big == len(T.SWEEP_MAX3) * U.PARTS3 and last_big >= U.PARTS3 * 4 and inner_big


def test_state_4_holds_refused_rows_between_owning_ones(oracle_mod):
    cfg = U.cfg4()
    with oracle_mod.OracleEngine(cfg) as ora:
        U.fill4(ora)
        for n in B.N4:
            _, want = T.model4(ora, n)
            res = want[1]
            kinds = [T.kind_of(res, r) for r in range(n)]
            assert all(k == "error" for k in kinds[6::7]) and "error" not in set(kinds) - set(kinds[6::7]) or n < 7
            if n >= 17:
                assert {"owning", "empty", "error"} <= set(kinds)
                r = kinds.index("error")
                assert "owning" in kinds[:r] and "owning" in kinds[r + 1:]
        _agrees_with_parse_records(want)  # the largest call


def test_expected_leaves_rows_that_do_not_fit_untouched(ora1):
    ora, cfg = ora1
    want = T.plain1(ora, 10)
    rec_row, rec_pos = T.table_of(want[1], want[2])
    need = int(rec_row[-1])
    owners = np.flatnonzero(T.words_of(want[1]))
    mid = int(owners[len(owners) // 2])
    for cap, rc in ((need, A.RMQ_OK), (need - 1, A.RMQ_ENOSPC), (int(rec_row[mid]) + 1, A.RMQ_ENOSPC), (0, A.RMQ_ENOSPC)):
        got_rc, row, left = T.expected(want, cap, alloc=need + 8)
        assert got_rc == rc and np.array_equal(row, rec_row)
        fits = int(max([rec_row[r + 1] for r in owners if rec_row[r + 1] <= cap], default=0))
        assert np.array_equal(left[:fits], rec_pos[:fits]) and (left[fits:] == T.SENT).all()


def test_reference_walk_is_bounded_on_damaged_length_words():
    rng = np.random.default_rng(5)
    lens = [600, 0, 17, 1500, 240]
    run = np.zeros(sum(16 + ((x + 15) & ~15) for x in lens), np.uint8)
    pos = 0
    for k, ln in enumerate(lens):
        run[pos:pos + 8] = np.frombuffer(int(100 + k).to_bytes(8, "little"), np.uint8)
        run[pos + 8:pos + 12] = np.frombuffer(int(ln).to_bytes(4, "little"), np.uint8)
        run[pos + 16:pos + 16 + ln] = rng.integers(0, 256, ln, dtype=np.uint8)
        pos += 16 + ((ln + 15) & ~15)
    clean = T.reference_walk(run, len(lens))
    assert np.array_equal(clean, T._scan(run, 100, len(lens), False, True)[2].astype(np.uint64))
    for bad in (0x58, 0xFFFFFFF0, 0xFFFFFFFF, 0):
        d = run.copy()
        d[8:12] = np.frombuffer(int(bad).to_bytes(4, "little"), np.uint8)
        w = T.reference_walk(d, len(lens))
        assert w[0] == 0 and w[-1] == run.size and not (w % 16).any() and (w <= run.size).all()
        assert not np.array_equal(w, clean)
