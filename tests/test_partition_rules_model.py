"""The case tables of tests/partition_rules_util.py through the independent model and the C oracle,
op by op, without a GPU: the two must agree on every state word and live index entry after every
batch and control call, the oracle must accept every table as written, and every table must really
hold the edges tests/test_gpu_partition_rules.py claims to run on the device (asserted from the
model's arithmetic alone, so no device test can pass by having nothing at its edge)."""
import numpy as np
import pytest

import partition_rules_util as U
from ripplemq_amd.engine import EngineConfig

S, I, ROOM = U.S, U.I, U.ROOM


def run_table(O, table, allowed=()):
    """Model and oracle through the table. Returns the trace: per op {"op", "states" (the model's,
    every partition, after the op), "stats" (one per batch of the op)}. `allowed` names the only
    rejection counters that may be non-zero."""
    cfg = EngineConfig(**table.cfg)
    P, G = cfg.num_partitions, cfg.pipeline_depth
    model = U.PartitionModel(P, cfg.replication_factor)
    icap = (2 * G + 2) * S // I
    trace, appended = [], 0
    with O.OracleEngine(cfg) as ora:
        for op in table.ops:
            steps = [("append", b) for b in op[1]] if op[0] == "pipelined" else [op]
            stats = []
            for step in steps:
                mres, ores = model.apply(step), U.apply_oracle(ora, step)  # (RMQ_EINVAL would raise)
                for (mo, ms), (oo, os_) in zip(mres, ores):
                    assert ms == os_, f"{table.name}: append stats model={ms} oracle={os_}"
                    assert mo == oo.tolist(), f"{table.name}: out offsets differ"
                    bad = {k: v for k, v in ms.items() if k.startswith("rejected") and v and k not in allowed}
                    assert not bad, f"{table.name}: rejections the table is not named for: {bad}"
                    stats.append(ms)
                    appended += ms["appended"]
                U.assert_model_agrees(model, ora, range(P), "oracle")
                for p in range(P):
                    lo, ent = model.live_index(p)
                    assert len(ent) <= icap, f"{table.name}: {len(ent)} live index entries, icap {icap}"
            trace.append({"op": op, "states": [model.state(p) for p in range(P)], "stats": stats})
    assert appended, f"{table.name}: nothing was appended"
    return trace


def holders(st):
    return sum(1 for m in st["match"] if m)


# ---- A ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("RF", range(1, 9))
def test_commit_rule_table(oracle_mod, RF):
    t = U.table_a(RF)
    n, k = t.notes, RF // 2 + 1
    P = len(n["masks"])
    tr = run_table(oracle_mod, t)
    acks = [i for i, e in enumerate(tr) if e["op"][0] == "ack"]

    if RF == 1:
        assert n["masks"] == [[0]]
        assert all(e["states"][0]["commit"] == e["states"][0]["log_end_offset"] for e in tr)
    else:
        # an ack after which exactly k - 1 slots hold a value and commit did not move, and the next
        # ack after which it moved to the k-th largest
        found = False
        for a, b in zip(acks, acks[1:]):
            for p in range(P):
                s0, s1, s2 = tr[a - 1]["states"][p], tr[a]["states"][p], tr[b]["states"][p]
                found |= (holders(s1) == k - 1 and s1["commit"] == s0["commit"] and holders(s2) == k
                          and s2["commit"] > s1["commit"]
                          and s2["commit"] == sorted(s2["match"], reverse=True)[k - 1])
        assert found, "no walk step crosses from k - 1 to k holders"
        # the term gate blocked (N > commit, N < term_start) and released at N == term_start
        gb, released = n["gate_below"], 0
        for p in range(P):
            before, s = tr[gb - 1]["states"][p], tr[gb]["states"][p]
            N = sorted(s["match"], reverse=True)[k - 1]
            if N > s["commit"] and N < s["term_start"]:
                assert s["commit"] == before["commit"] and N == s["term_start"] - 1
                after = tr[n["gate_at"]]["states"][p]
                assert sorted(after["match"], reverse=True)[k - 1] == after["term_start"] == after["commit"]
                released += 1
        assert released, "the gate never blocked"
        # a partition that one ack at term_start releases, and one that needs more of them
        if RF > 3:
            first = [tr[n["gate_first"]]["states"][p]["commit"] == 26 for p in range(P) if len(n["masks"][p]) < k]
            assert any(first) and not all(first)
        # the clamp
        c = n["clamp"]
        for p, r, v in zip(*tr[c]["op"][1:4]):
            assert v > tr[c]["states"][p]["log_end_offset"] == tr[c]["states"][p]["match"][r] == 20
        # nothing goes back
        for key in ("no_regress",):
            assert tr[n[key]]["states"] == tr[n[key] - 1]["states"]
            assert all(v < tr[n[key]]["states"][p]["match"][r] for p, r, v in zip(*tr[n[key]]["op"][1:4]))
        # the new term: remote matches 0, term_start the log end, commit only moves with a local quorum
        t3 = n["term3"] + P - 1
        for p in range(P):
            before, s = tr[n["term3"] - 1]["states"][p], tr[t3]["states"][p]
            assert s["term"] == 3 and s["term_start"] == s["log_end_offset"] == 26
            assert all(s["match"][r] == 0 for r in n["remote"][p])
            quorum = len(n["masks"][p]) >= k
            assert s["commit"] == (26 if quorum else before["commit"])
            assert quorum or before["commit"] < 26
    # acks to a local slot, lower and higher: nothing moves
    for key in ("local_low", "local_high"):
        assert tr[n[key]]["states"] == tr[n[key] - 1]["states"]
    # the same (partition, slot) three times, in two orders: the maximum wins
    for i, top in zip(n["dup"], (13, 16)):
        items = list(zip(*tr[i]["op"][1:4]))
        assert len(items) == 3 * P and len(set((p, r) for p, r, _ in items)) == P
        for p, r, _ in items:
            assert tr[i]["states"][p]["match"][r] == max(tr[i - 1]["states"][p]["match"][r], top)
    assert [v for _, _, v in zip(*tr[n["dup"][0]]["op"][1:4])][:3] == [11, 13, 12]
    assert [v for _, _, v in zip(*tr[n["dup"][1]]["op"][1:4])][::P] == [16, 14, 15]
    # the long call: past the control area, every pair many times, the clamped maximum per slot
    lg = n["long"]
    items = list(zip(*tr[lg]["op"][1:4]))
    assert len(items) >= 1100 and len(items) > 1024 + 64
    best = {}
    for p, r, v in items:
        best[(p, r)] = max(best.get((p, r), 0), v)
    assert set(best) == {(p, r) for p in range(P) for r in range(RF)}
    assert min(sum(1 for p, r, _ in items if (p, r) == pr) for pr in best) >= 3
    assert any(v > 20 for v in best.values())
    for (p, r), v in best.items():
        assert tr[lg]["states"][p]["match"][r] == max(tr[lg - 1]["states"][p]["match"][r], min(v, 20))
    # back-to-back appends: a local quorum commits on append, the others do not
    pipes = [i for i, e in enumerate(tr) if e["op"][0] == "pipelined"]
    assert len(pipes) == 2
    for i in pipes:
        for p in range(P):
            s = tr[i]["states"][p]
            assert (s["commit"] == s["log_end_offset"]) == (len(n["masks"][p]) >= k), (i, p, s)
    assert tr[-1]["states"][0]["log_end_offset"] == n["leo"]
    assert all(s["log_start_offset"] == 0 for s in tr[-1]["states"])  # (no table A ring wraps)


def test_masks_of_table_a():
    assert U.masks_for(1) == [[0]]
    assert U.masks_for(2) == [[0], [1], [0, 1]]
    assert U.masks_for(3) == [[0], [2], [0, 2], [0, 1, 2]]
    assert U.masks_for(8) == [[0], [7], [0, 1, 2, 3], [0, 4, 5, 6, 7], list(range(8))]
    for RF in range(3, 9):
        k = RF // 2 + 1
        m = U.masks_for(RF)
        assert {len(x) for x in m} == {1, k - 1, k, RF}
        quorum = [x for x in m if len(x) == k]
        assert len(quorum) == 1 and any(b - a > 1 for a, b in zip(quorum[0], quorum[0][1:]))  # not contiguous
        assert U.ranks_of(m[1], RF) == [r + 1 for r in range(RF - 1)] + [0]


# ---- B ----------------------------------------------------------------------------------------

def test_space_rule_table(oracle_mod):
    t = U.table_b()
    p, q = t.notes["p"], t.notes["q"]
    tr = run_table(oracle_mod, t, allowed=("rejected_no_space",))
    assert len(tr) == len(t.notes["names"]) == 8
    for k, (name, e) in enumerate(zip(t.notes["names"], tr)):
        b, st = e["op"][1], e["stats"][0]
        np_, nq = int((b.pidx == p).sum()), int((b.pidx == q).sum())
        assert abs(np_ - nq) <= 1 and b.pidx[0] == p and b.pidx[1] == q  # record by record
        before = tr[k - 1]["states"][p]["log_end_pos"] if k else 0
        if name.startswith("fit"):
            assert U.bytes_for(b, p) == ROOM == 3840
            assert st["rejected_no_space"] == 0 and st["appended"] == np_ + nq
            assert e["states"][p]["log_end_pos"] == before + ROOM
        else:
            assert U.bytes_for(b, p) == ROOM + 16
            assert st["rejected_no_space"] == np_ and st["appended"] == nq
            assert e["states"][p]["log_end_pos"] == before
        if "unequal" in name:
            lens = b.lens[b.pidx == p]
            assert (lens == 0).sum() >= 3 and len(set(lens.tolist())) >= 6
        if "wrapped" in name:
            assert before > S and tr[k - 1]["states"][p]["log_start_offset"] > 0


# ---- C ----------------------------------------------------------------------------------------

def test_retention_threshold_table(oracle_mod):
    t = U.table_c()
    n = t.notes
    tr = run_table(oracle_mod, t)

    def st(i, p):
        return tr[i]["states"][p]

    # end - start == S: the start stays; 16 bytes more: it moves; the same from a moved start
    for full, move in ((n["full0"], n["move0"]), (n["full1"], n["move1"])):
        a, b = st(full, 0), st(move, 0)
        assert a["log_end_pos"] - a["log_start_pos"] == S
        assert a["log_start_pos"] == st(full - 1, 0)["log_start_pos"]
        assert b["log_end_pos"] == a["log_end_pos"] + 16 and b["log_start_pos"] > a["log_start_pos"]
    assert st(n["full0"], 0)["log_start_pos"] == 0 and st(n["move0"], 0)["log_start_pos"] == 288
    assert st(n["full1"], 0)["log_start_pos"] == 288 and st(n["move1"], 0)["log_start_pos"] == 528
    # the two sides of the ceil, and both kinds of E[m*]
    s1, s2, s3 = st(n["ceil1"], 1), st(n["ceil2"], 2), st(n["ceil3"], 3)
    assert s1["log_end_pos"] - S == I and s2["log_end_pos"] - S == I + 16
    assert (s1["log_start_offset"], s1["log_start_pos"]) == (4, I)        # a record ends on m* I
    assert (s2["log_start_offset"], s2["log_start_pos"]) == (8, 2 * I)
    assert s3["log_end_pos"] - S == I and s3["log_start_pos"] == 288 > I  # a record straddles m* I
    # the split pair: the same records, other batch boundaries, other log starts (§4)
    a, b = st(n["split_a"], 4), st(n["split_b"], 5)
    assert a["log_end_pos"] == b["log_end_pos"] and a["log_end_offset"] == b["log_end_offset"]
    lens = lambda op: [x for bt in (op[1] if op[0] == "pipelined" else [op[1]]) for x in bt.lens.tolist()]
    assert lens(t.ops[n["split_a"] - 1]) + lens(t.ops[n["split_a"]]) == \
        lens(t.ops[n["split_b"] - 1]) + lens(t.ops[n["split_b"]])
    assert a["log_start_pos"] == 288 and b["log_start_pos"] == 528
    assert a["log_end_pos"] - a["log_start_pos"] == S  # the last batch of the split sat on the threshold
    # both batches of the split share a launch group of the device engine
    assert t.ops[n["split_a"]][0] == "pipelined" and len(t.ops[n["split_a"]][1]) == t.cfg["pipeline_depth"] == 2


def test_split_pair_alone(oracle_mod):
    # retention evaluated per launch group, or per call order, instead of per batch fails here
    t = U.table_c_split()
    tr = run_table(oracle_mod, t)
    a, b = tr[t.notes["split_a"]]["states"][4], tr[t.notes["split_b"]]["states"][5]
    assert a["log_end_pos"] == b["log_end_pos"] == S + 288
    assert (a["log_start_offset"], a["log_start_pos"]) == (6, 288)
    assert (b["log_start_offset"], b["log_start_pos"]) == (11, 528)


# ---- D ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("G", U.DEPTHS)
@pytest.mark.parametrize("name", U.D_CASES)
def test_group_tables(oracle_mod, name, G):
    allowed = {"middle_refused": ("rejected_no_space",), "not_led": ("rejected_not_leader",)}.get(name, ())
    for order in U.ORDERS:
        t = U.table_d(name, G, order)
        case = t.notes["case"]
        tr = run_table(oracle_mod, t, allowed)
        batches = tr[-1]["op"][1]
        nb, total = len(case.batches), len(batches)
        assert all((b.pidx == U.Q_D).sum() >= 3 for b in batches)  # every batch moves q's log end
        assert tr[-1]["states"][U.Q_D]["log_end_offset"] == 3 * (total + sum(op[0] == "append" for op in case.pre))
        if order == "read":  # the case's last group and two more are closed
            assert total == (-(-nb // G) + 2) * G and all(U.bytes_for(b, U.P_D) == 0 for b in batches[nb:])
        elif order == "sync":
            assert total == nb
        else:                # the case's last group is full and one whole group follows
            assert total == (-(-nb // G) + 1) * G
            assert all(U.bytes_for(b, U.P_D) == (64 if order == "next_with_p" else 0) for b in batches[nb:])
        late, moved = U.late_batches(case, batches[nb:])
        assert all(j < -(-nb // G) * G for j in late)  # the groups after the case's are never late themselves
        if order == "sync":
            check_late_formula(name, G, case, late, moved, tr[-1])


def check_late_formula(name, G, case, late, moved, last):
    """Which batches the launch cannot retain, by §4 and the read limit alone."""
    nb = len(case.batches)
    by_p = [U.bytes_for(b, U.P_D) for b in case.batches]
    if G == 1:
        assert late == []  # a batch adds at most S - I: its entry lies below the log end before it
    if name == "two_full":
        assert by_p == [ROOM, ROOM]
        assert late == ([1] if G > 1 else []) and moved == [1]
        assert -(-(2 * ROOM - S) // I) * I > 0  # ceil((fin_2 - S) / I) I > used0 = 0
    if name.startswith("pair_"):
        X = sum(by_p)
        assert all(0 < x <= ROOM for x in by_p) and moved == [1]
        used0 = 4 * I
        need = -(-(used0 + X - S) // I) * I
        if name == "pair_past_ring":
            assert X == S + 16 and need == used0 + I
            assert late == ([1] if G > 1 else [])
        else:
            assert ROOM < X <= S and need == used0  # the entry sits exactly at the log end before
            assert late == []
    if name == "g_full":
        assert by_p == [ROOM] * G and moved == list(range(1, G))
        assert late == list(range(1, G))
        if G == 8:
            assert len(moved) >= 6 and sum(by_p) == 7 * S + S // 2  # seven and a half rings
    if name == "middle_empty":
        assert by_p == [ROOM, 0, ROOM] and moved == [2]
        assert late == ([2] if G >= 3 else [])
    if name == "middle_refused":
        assert by_p == [ROOM, ROOM + 16, ROOM] and moved == [2]
        assert last["stats"][1]["rejected_no_space"] == (ROOM + 16) // 16
        assert late == ([2] if G >= 3 else [])
    if name == "not_led":
        assert not case.led and late == [] and moved == []
        assert last["states"][U.P_D]["log_end_offset"] == 0 and last["states"][U.P_D]["is_leader"] == 0
        assert last["stats"][0]["rejected_not_leader"] == ROOM // 64
    else:
        assert last["states"][U.P_D]["log_end_pos"] > 0


def test_the_boundary_pair_is_one_late_and_one_not():
    for G in (2, 3, 8):
        at = U.late_batches(U.group_case("pair_at_ring", G))[0]
        room = U.late_batches(U.group_case("pair_past_room", G))[0]
        past = U.late_batches(U.group_case("pair_past_ring", G))[0]
        assert (at, room, past) == ([], [], [1])
    for G in U.DEPTHS:  # whether the last group of a case is late: some are and some are not, none at G = 1
        last = {}
        for nm in U.D_CASES:
            case = U.group_case(nm, G)
            first = (len(case.batches) - 1) // G * G
            last[nm] = any(j >= first for j in U.late_batches(case)[0])
        assert any(last.values()) == (G > 1) and not all(last.values()), (G, last)


# ---- E ----------------------------------------------------------------------------------------

def test_many_partitions_table(oracle_mod):
    t = U.table_e()
    tr = run_table(oracle_mod, t)
    assert t.cfg["num_partitions"] == 600 == 2 * 256 + 88 and t.cfg["replication_factor"] == 8
    assert {tuple(U.mask_e(p)) for p in range(600)} == {tuple(m) for m in U.E_MASKS}
    last = tr[-1]["states"]
    assert len({s["commit"] for s in last}) > 2 and len({s["log_end_offset"] for s in last}) > 2
    assert any(s["commit"] < s["log_end_offset"] for s in last) and all(s["term"] == 3 for s in last)
    for first, n in U.E_RANGES:
        assert 0 <= first and first + n <= 600
