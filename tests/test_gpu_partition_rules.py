"""The partition rules at their edges on the device: the case tables of tests/partition_rules_util.py
through the HIP engine and the C oracle (tests/parity.py: offsets, stats, state, whole rings, live
index entries, bit for bit), with the independent model of the same file as a third party on the
state words and index entries. tests/test_partition_rules_model.py proves without a GPU that the
tables hold the edges they are named for.

A: quorum commit at every RF from 1 to 8 and every local-slot mask, the rmq_ack clamp, duplicates
and a call past the control area, the current-term gate. B: the space rule at S - I and S - I + 16.
C: retention at end - start == S, both sides of the ceil, both kinds of E[m*], batch boundaries.
D: launch groups whose retention replay stops in the launch, finished by each of the three pieces
of code that can finish it. E: leader start and bulk state reads over 600 partitions."""
import numpy as np
import pytest

import partition_rules_util as U
from parity import compare_bulk, compare_state, run_ops
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine, EngineConfig

pytestmark = pytest.mark.gpu


def run_table(oracle_mod, table):
    cfg = EngineConfig(**table.cfg)
    P = cfg.num_partitions
    model = U.PartitionModel(P, cfg.replication_factor)
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        for k, op in enumerate(table.ops):
            try:
                run_ops(dev, ora, cfg, [op], full_rings=True, local_slots=table.local_slots)
                model.apply(op)
                U.assert_model_agrees(model, dev, range(P), "gpu")
            except AssertionError as ex:
                raise AssertionError(f"{table.name} op {k} ({op[0]}): {ex}") from ex
        compare_state(dev, ora, cfg, full_rings=True, local_slots=table.local_slots)


@pytest.mark.parametrize("RF", range(1, 9))
def test_commit_rule(oracle_mod, RF):
    run_table(oracle_mod, U.table_a(RF))


def test_space_rule(oracle_mod):
    run_table(oracle_mod, U.table_b())


def test_retention_threshold(oracle_mod):
    run_table(oracle_mod, U.table_c())


def _fetch_both(dev, ora, consumer):
    pp = np.array([U.P_D, U.Q_D], np.uint32)
    cc = np.full(2, consumer, np.uint32)
    mx = np.full(2, 1 << 20, np.uint32)
    rd, res, buf, ud = dev.fetch(pp, cc, mx)
    ro, want, wbuf, uo = ora.fetch(pp, cc, mx)
    assert (rd, ud) == (ro, uo)
    for k in ("status", "start_offset", "count", "bytes"):
        assert np.array_equal(res[k], want[k]), (k, res[k], want[k])
    assert np.array_equal(buf[:ud], wbuf[:uo]), "fetched bytes differ"
    return want


@pytest.mark.parametrize("order", U.ORDERS)
@pytest.mark.parametrize("G", U.DEPTHS)
@pytest.mark.parametrize("name", U.D_CASES)
def test_groups_and_late_retention(oracle_mod, name, G, order):
    """Every batch is submitted before any is waited for. read: the state and a fetch from offset 0
    right after the submissions, without a sync (late_retention_kernel finishes the replay); sync:
    a sync at once (the stage-4-only launch of the drain); next_*: a further group first (stage 4 of
    its launch)."""
    t = U.table_d(name, G, order)
    case = t.notes["case"]
    cfg = EngineConfig(**t.cfg)
    model = U.PartitionModel(2, cfg.replication_factor)
    batches = t.ops[-1][1]
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        for op in case.pre:
            run_ops(dev, ora, cfg, [op], full_rings=True)
            model.apply(op)
        subs = [dev.append_async(b.pidx, b.lens, b.payload) for b in batches]
        want = []

        def advance():
            b = batches[len(want)]
            want.append(ora.append(b.pidx, b.lens, b.payload))
            model.append(b.pidx, b.lens)

        if order == "read":
            st = [dev.state(p) for p in range(2)]
            leo = [s["log_end_offset"] for s in st]
            while [ora.state(p)["log_end_offset"] for p in range(2)] != leo:
                assert len(want) < len(batches), "device state matches no prefix of the batches"
                advance()
            # the launch that applies the case's last group was issued before the read
            assert len(want) >= len(case.batches), f"only {len(want)} batches applied at the read"
            assert st == [ora.state(p) for p in range(2)], f"state after {len(want)} applied batches"
            U.assert_model_agrees(model, dev, range(2), "gpu")
            res = _fetch_both(dev, ora, 0)
            start = ora.state(U.P_D)["log_start_offset"]
            if start:  # below the start: RMQ_EOFFSET, naming the first retained offset
                assert res["status"][0] == A.RMQ_EOFFSET and res["start_offset"][0] == start
                for e in (dev, ora):
                    e.commit_consumer_offset([U.P_D, U.Q_D], [1, 1], [start, 0])
                res = _fetch_both(dev, ora, 1)
                assert res["status"][0] == A.RMQ_OK and res["count"][0] > 0
        dev.sync()
        while len(want) < len(batches):
            advance()
        for k, ((tk, out), (oo, so)) in enumerate(zip(subs, want)):
            sd = dev.wait(tk)
            assert sd == so, f"batch {k}: append stats gpu={sd} cpu={so}"
            assert np.array_equal(out, oo), f"batch {k}: out offsets differ"
        compare_state(dev, ora, cfg, full_rings=True)
        U.assert_model_agrees(model, dev, range(2), "gpu")
        if case.led:
            assert dev.state(U.P_D)["log_end_pos"] > 0
            late, moved = U.late_batches(case, batches[len(case.batches):])
            assert bool(moved) == (dev.state(U.P_D)["log_start_offset"] > 0)


@pytest.mark.parametrize("G", U.DEPTHS)
@pytest.mark.parametrize("name", U.D_CASES)
def test_drain_adds_a_stage4_launch_exactly_for_late_groups(monkeypatch, capfd, name, G):
    """That the late cases reach the code they are meant for: with RMQ_TRACE=1 the engine prints every
    pipeline launch's roles ("rmq launch <n>: ... | s3 <b> batches ... | s4 <b> batches").
    A sync right after the submissions ends with a launch that applies nothing and carries the last
    group as stage 4 exactly when U.late_batches, the formula alone, names a batch of that group."""
    import re
    monkeypatch.setenv("RMQ_TRACE", "1")
    case = U.group_case(name, G)
    cfg = EngineConfig(**U.base_cfg(2, 3, G))
    with Engine(cfg) as dev:
        for op in case.pre:
            U.apply_oracle(dev, op)
        capfd.readouterr()
        for b in case.batches:
            dev.append_async(b.pidx, b.lens, b.payload)
        dev.sync()
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rmq launch")]
    roles = [tuple(int(x) for x in re.search(r"s3 (\d+) batches.*s4 (\d+) batches", ln).groups()) for ln in lines]
    nb = len(case.batches)
    last = (nb - 1) // G * G  # the first batch of the last group
    assert sum(s3 for s3, _ in roles) == nb, lines
    late = [j for j in U.late_batches(case)[0] if j >= last]
    assert (roles[-1] == (0, nb - last)) == bool(late), (late, lines)
    assert late or roles[-1][0] == nb - last, lines


def test_many_partitions_leader_start_and_bulk_reads(oracle_mod):
    t = U.table_e()
    cfg = EngineConfig(**t.cfg)
    P = cfg.num_partitions
    model = U.PartitionModel(P, cfg.replication_factor)
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        for op in t.ops:
            if op[0] == "set_placement":
                for e in (dev, ora):
                    e.set_placement(op[1], None, op[2], op[3])
            else:
                run_ops(dev, ora, cfg, [op], check=False)
            model.apply(op)
            if op[0] == "become_leader":  # three blocks of 256 threads, a tail of 88
                sd, so = dev.states(0, P), ora.states(0, P)
                assert sd.tobytes() == so.tobytes(), f"states differ after become_leader at term {op[2]}"
        for first, n in U.E_RANGES:
            sd, so = dev.states(first, n), ora.states(first, n)
            for i in range(n):
                assert sd[i].tobytes() == so[i].tobytes(), f"states({first}, {n})[{i}]\n gpu={sd[i]}\n cpu={so[i]}"
            ones = dev.states(first, 1) if n == 1 else None
            for i in range(n):  # the bulk gather against one partition at a time
                one = dev.state(first + i)
                for f in U.STATE_KEYS:
                    got = sd[i][f].tolist()
                    got = got[:cfg.replication_factor] if f == "match" else int(got)
                    assert got == one[f], f"states({first}, {n})[{i}].{f}: {got}, state(): {one[f]}"
            assert ones is None or ones.tobytes() == sd.tobytes()
        U.assert_model_agrees(model, dev, range(P), "gpu")
        compare_bulk(dev, ora, cfg, local_slots=t.local_slots)
