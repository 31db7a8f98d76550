"""CPU proof that the device-batch sweep (tests/test_gpu_append_device.py) is not vacuous: every case
table of tests/device_batch_util.py holds the classes it is named for (classify: lengths x start
residues, store paths per task, staged and unstaged spans, the 256 / 257 block edge, task and tile
tails), at every payload shift the GPU test uses, and the oracle alone appends every record of every
valid table (no rejection for space: the rings hold the tables). The invalid tables are refused by
the oracle's range_check and name no byte outside what DeviceBatch allocates."""
import numpy as np
import pytest

import device_batch_util as D
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import EngineError


@pytest.mark.parametrize("order", D.ORDERS)
@pytest.mark.parametrize("make", [D.explicit_table, D.packed_table])
def test_length_tables_hold_every_length_at_every_residue(make, order):
    case = make(order)
    assert case.batch.n <= D.MAX_RECS
    for shift in D.SHIFTS:
        got = D.classes(case.batch, shift, case.poff)
        assert not case.expect - got, (case.name, shift, sorted(case.expect - got))
        # 22 lengths x 16 residues
        assert len({c for c in got if c.startswith("L")} & case.expect) == 16 * len(D.LENS)
    if case.poff is not None:  # gaps, and no payload overlaps the next one
        ends = case.poff.astype(np.int64) + case.batch.lens
        assert (case.poff[1:].astype(np.int64) >= ends[:-1]).all() and ends[-1] == case.batch.payload.size


def test_sorted_tables_have_homogeneous_tasks_and_permuted_ones_mixed():
    for make in (D.explicit_table, D.packed_table):
        paths = {}
        for order in D.ORDERS:
            case = make(order)
            c = D.classify(case.batch, 0, case.poff)
            paths[order] = [t["path"] for t in c["tasks"]]
            kinds = [len(set(case.batch.lens[t["i0"]:t["i0"] + t["n"]])) for t in c["tasks"][:-3]]
            if order == "permuted":  # every task mixes lengths; short, long and large records share tasks
                assert min(kinds) >= 6 and any(t["long"] and t["bigs"] and t["long"] + t["bigs"] < t["n"]
                                               for t in c["tasks"]), case.name
            else:  # (a packed task: 16 fillers of 0..15 B and 16 records of one length)
                assert max(kinds) <= (1 if case.poff is not None else 17), case.name
            pure = sum(1 for t in c["tasks"] if t["n"] == D.TASK_RECS and t["path"] == "image")
            assert pure >= 1 or order == "permuted", (case.name, "a task of 32 image records")
            assert {"one_long", "one_big"} <= D.classes(case.batch, 0, case.poff)
        # sorted: runs of tasks of one path, in the order image, piecewise, big (before the crafted tasks)
        body = paths["sorted"][:-3]
        assert body == sorted(body, key=["image", "piecewise", "big"].index) and len(set(body)) == 3


def test_explicit_sorted_tasks_hold_one_length():
    case = D.explicit_table("sorted")
    for t in D.classify(case.batch, 0, case.poff)["tasks"][:len(D.LENS)]:
        assert len(set(case.batch.lens[t["i0"]:t["i0"] + t["n"]])) == 1


def test_span_and_tail_cases_hold_their_edges():
    seen = set()
    for case, shift in D.span_cases():
        got = D.classes(case.batch, shift)
        assert not case.expect - got, (case.name, shift, case.expect - got)
        seen |= got
    assert {"blocks256:staged", "blocks257:unstaged", "empty_span"} <= seen
    tails = set()
    for n in D.TAIL_COUNTS:
        case = D.tail_case(n)
        got = D.classes(case.batch, 0)
        assert not case.expect - got, (case.name, case.expect - got)
        assert case.declared is None and case.batch.payload.size == 100 * n  # declared: the exact size
        tails.add((n % D.TASK_RECS, n % D.TILE_RECS))
        # 32 x 100 B: every full task's span is staged
        assert all(t["staged"] for t in D.classify(case.batch, 0)["tasks"])
    assert {(1, 1), (0, 0), (31, 1023), (1, 1)} <= tails and {r for r, _ in tails} >= {0, 1, 2, 31}
    m = D.mixed40()
    assert m.batch.n == 40 and {"tail_task"} <= D.classes(m.batch, 0) and len(set(m.batch.lens)) > 8


def test_thresholds_sit_between_the_table_lengths():
    # 7 / 8 pieces, one / two load rounds, 64 / 65 pieces: each edge has a length on both sides
    pieces = lambda L: -(-L // 16)
    assert pieces(112) == D.IMG_PIECES and pieces(113) == D.IMG_PIECES + 1
    assert pieces(128) == D.ROUND_PIECES and pieces(129) == D.ROUND_PIECES + 1
    assert pieces(1024) == D.BIG_PIECES and pieces(1025) == D.BIG_PIECES + 1
    assert {112, 113, 128, 129, 1024, 1025} <= set(D.LENS)


def _oracle_takes(oracle_mod, ora, case):
    b = case.batch
    declared = b.payload.size if case.declared is None else case.declared
    return ora.append(b.pidx, b.lens, b.payload[:declared], case.poff)


def test_oracle_appends_every_record_of_the_valid_tables(oracle_mod):
    cases = D.length_tables() + [c for c, _ in D.span_cases()] + [D.tail_case(n) for n in D.TAIL_COUNTS]
    cases += [D.mixed40(), D.packed_range_case(D.RANGE_N, 0), D.packed_range_case(33, 0)]
    for case in cases:
        with oracle_mod.OracleEngine(D.small_config()) as ora:
            for _ in range(8):  # (the GPU test's eight passes: the length tables wrap the rings)
                _, st = _oracle_takes(oracle_mod, ora, case)
                assert st["appended"] == case.batch.n and st["rejected_no_space"] == 0, (case.name, st)
            if case.name.startswith(("explicit-", "packed-")):
                assert max(ora.state(p)["log_start_offset"] for p in range(D.P)) > 0, case.name
    with oracle_mod.OracleEngine(D.small_config()) as ora:
        case = D.explicit_range_case()
        _, st = _oracle_takes(oracle_mod, ora, case)
        assert st == {"records": case.batch.n, "appended": case.batch.n - 1, "rejected_not_leader": 0,
                      "rejected_no_partition": 1, "rejected_no_space": 0, "rejected_invalid": 0}


def test_invalid_tables_break_the_rule_by_one_byte(oracle_mod):
    bad = [D.explicit_range_case(k, p) for k in D.RANGE_KINDS for p in D.RANGE_PLACES]
    bad += [D.packed_range_case(D.RANGE_N, 1), D.packed_range_case(33, 1)]
    valid = D.explicit_range_case()
    for case in bad:
        assert case.invalid
        b = case.batch
        with oracle_mod.OracleEngine(D.small_config()) as ora:
            with pytest.raises(EngineError) as ex:
                _oracle_takes(oracle_mod, ora, case)
            assert ex.value.status == A.RMQ_EINVAL, case.name
        start = D.record_starts(b, case.poff)
        over = start + b.lens - case.declared
        if case.poff is not None:
            # one record differs from the valid table, and it ends one byte past payload_bytes
            diff = np.flatnonzero((case.poff != valid.poff) | (b.lens != valid.batch.lens))
            assert len(diff) == 1 and over[diff[0]] in (1, 2) and b.lens[diff[0]] > 0, case.name
            assert ((over <= 0) | (b.lens == 0))[np.arange(b.n) != diff[0]].all()
            k = int(diff[0])
            want_tile = 1 if "tile1" in case.name else 0
            assert k // D.TILE_RECS == want_tile and (b.pidx[k] >= D.P) == ("no_partition" in case.name)
        else:
            assert int(b.lens.sum()) == case.declared + 1
        # DeviceBatch's invariant: the named ranges end within 16 bytes of the payload array's end
        assert int((start + b.lens).max()) <= b.payload.size + 2
    # the edges the rule allows are in the valid table, in both tiles
    o, L, Dd = valid.poff.astype(np.int64), valid.batch.lens.astype(np.int64), valid.declared
    for tile in (0, 1):
        sl = slice(tile * D.TILE_RECS, (tile + 1) * D.TILE_RECS)
        assert ((o[sl] + L[sl] == Dd) & (L[sl] > 0)).any()
        assert ((o[sl] == Dd) & (L[sl] == 0)).any() and ((o[sl] == Dd + 1) & (L[sl] == 0)).any()
