"""The ring-move scenarios of tests/ring_move_util.py on the CPU oracle alone: every guard a scenario
relies on (which chunks and index shares of a move hold live data, which block a grow must reuse,
where a shrink's new log start falls, ...) is asserted here on oracle state, so a scenario that has
become vacuous fails without a GPU. tests/test_gpu_ring_moves.py runs the same scenarios through
the HIP engine and compares it with the oracle byte for byte."""
import numpy as np
import pytest

import ring_move_util as U
from ripplemq_amd import _abi as A

KiB = U.KiB


def run(oracle_mod, scn):
    with oracle_mod.OracleEngine(scn.cfg) as ora:
        snaps = U.play(scn, ora)
        assert set(scn.guards) <= set(snaps), "a guard names no stage"
    return snaps


def test_builders_are_deterministic():
    a, b = U.multi_chunk_grow(512 * KiB), U.multi_chunk_grow(512 * KiB)
    for (na, oa), (nb, ob) in zip(a.stages, b.stages):
        assert na == nb and len(oa) == len(ob)
        for x, y in zip(oa, ob):
            if x[0] == "append":
                assert all(np.array_equal(p, q) for p, q in ((x[1].pidx, y[1].pidx), (x[1].lens, y[1].lens),
                                                               (x[1].payload, y[1].payload)))


@pytest.mark.parametrize("new_seg", [512 * KiB, 1 << 20])
def test_multi_chunk_grow_guards(oracle_mod, new_seg):
    scn = U.multi_chunk_grow(new_seg)
    assert U.chunks_of(new_seg) == new_seg // U.MIGRATE_CHUNK in (2, 4)
    run(oracle_mod, scn)


def test_dirty_block_reuse_guards(oracle_mod):
    run(oracle_mod, U.dirty_block_reuse())


def test_mixed_items_guards(oracle_mod):
    run(oracle_mod, U.mixed_items())


@pytest.mark.parametrize("new_seg", [1 * KiB, 2 * KiB, 4 * KiB, 8 * KiB])
def test_shrink_edges_guards(oracle_mod, new_seg):
    scn = U.shrink_edges(new_seg)
    assert new_seg >= 4 * scn.cfg.index_interval
    assert sorted(k for k, _ in scn.facts["parts"].values()) == sorted(U.EDGE_KINDS * 2)
    run(oracle_mod, scn)


def test_shrink_misc_guards(oracle_mod):
    run(oracle_mod, U.shrink_misc())


def test_fetch_across_moves_guards(oracle_mod):
    scn = U.fetch_across_moves()
    with oracle_mod.OracleEngine(scn.cfg) as ora:
        # what the reads answer on the way: the evicted offset RMQ_EOFFSET and no record
        statuses = []
        for name, ops in scn.stages:
            for op in ops:
                if op[0] == "fetch":
                    _, res, _, _ = ora.fetch(op[1], op[2], op[3], None, commit=True)
                    statuses.append((name, int(res["status"][0]), int(res["count"][0])))
                else:
                    U.apply_ops(ora, [op])
        assert [s[1:] for s in statuses if s[0] == "resume"] == [(A.RMQ_EOFFSET, 0)], statuses
        assert all(s[1:] == (A.RMQ_OK, 10) for s in statuses if s[0] in ("read1", "read2", "read3")), statuses
        tail = [s[2] for s in statuses if s[0] == "read4"]
        assert all(s[1] == A.RMQ_OK for s in statuses if s[0] == "read4") and tail[0] == 10 and tail[-1] == 0, statuses
    run(oracle_mod, scn)


@pytest.mark.parametrize("depth,late", [(2, False), (3, False), (3, True)])
def test_pipelined_moves_guards(oracle_mod, depth, late):
    run(oracle_mod, U.pipelined_moves(depth, late))


def test_refused_calls_on_the_oracle(oracle_mod):
    scn = U.refused_calls()
    cfg = scn.cfg
    with oracle_mod.OracleEngine(cfg) as ora:
        U.apply_ops(ora, scn.stages[0][1])

        def everything():
            return ([ora.state(p) for p in range(cfg.num_partitions)],
                    [ora.read_segment(r, p).tobytes() for p in range(cfg.num_partitions)
                     for r in range(cfg.replication_factor)])

        before = everything()
        for name, pidx, sizes, status, judged in scn.facts["calls"]:
            if judged:
                assert U.call_status(ora, pidx, sizes) == status, name
                assert everything() == before, name
        assert {c[0] for c in scn.facts["calls"] if not c[4]} == {"above_pool"}
    run(oracle_mod, scn)


def test_follower_with_another_ring_size_on_the_oracles(oracle_mod):
    fs = U.follower_ring_script()
    assert [m is not None for m in fs.moves] == [True, True, False]
    oras = [oracle_mod.OracleEngine(c) for c in fs.cfgs]
    try:
        U.run_follower_oracles(oras, fs)
        U.follower_guards(oras, fs)
        led1 = [oras[1].state(p)["segment_bytes"] for p in range(fs.ppr)]
        fol1 = [oras[1].state(p)["segment_bytes"] for p in range(fs.ppr, len(fs.views[1].gp))]
        assert set(led1) == {512 * KiB} and set(fol1) == {32 * KiB}
    finally:
        for o in oras:
            o.close()
