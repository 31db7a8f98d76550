"""Differential sweep of the follower ingest (ripplemq_amd/csrc/replicate.hip) and of the transport
build of the append pipeline that fills the outboxes: engines on one GPU over the in-process
transport, in lock step with per-rank oracles (tests/ingest_util.py). After every round the regions
both ways (unmasked, the flipped byte included), the six replication counters and every rank's
digest (bulk states, consumer offsets, live index entries, the whole ring of every local slot) must
equal the oracle's. tests/test_ingest_states.py proves on the CPU that the scenarios hold the
lengths, fields, phases and task edges they are named for, and that every flip changes the digest.
"""
import numpy as np
import pytest

import ingest_util as X

pytestmark = pytest.mark.gpu


def sweep(oracle_mod, sc):
    ora = X.run_oracle(oracle_mod, sc)  # plans the flips: their bytes drive rmq_fault_corrupt below
    gpu = X.run_gpu(sc, ora.flips)
    X.compare_runs(sc, gpu, ora)
    flips = sum(len(f) for f in gpu.flips)
    last = gpu.counters[-1]
    print(f"\n{sc.name}: {sc.rounds} rounds, {flips} flips, refused crc/log {sum(c[1] for c in last)}/{sum(c[2] for c in last)}, "
          f"catch-up entries {sum(c[4] for c in last)}, records ingested {sum(c[0] for c in last)}")
    return ora, gpu


def caught_up(sc, gpu):
    views = sc.views()
    for r in range(sc.world):
        st = gpu.digests[-1][r]["states"]
        for p in range(views[r].led):
            assert [int(x) for x in st[p]["match"][:sc.rf]] == [int(st[p]["log_end_offset"])] * sc.rf, (sc.name, r, p)


@pytest.fixture(params=["default_grid", "one_workgroup"])
def verify_grid(request, monkeypatch):
    # RMQ_VERIFY_WGS is read when an engine is created: one workgroup's 8 waves then stride over all
    # the verify tasks of a round
    if request.param == "one_workgroup":
        monkeypatch.setenv("RMQ_VERIFY_WGS", "1")
    return request.param


def test_length_edges_over_the_link(oracle_mod, verify_grid):
    # A: every length of LENS_I through the transport build of the append kernel, the outbox fill,
    # ingest_verify and ingest_copy, five rounds of about 148 KB per partition into 512 KiB rings
    sc = X.scenario_a()
    _, gpu = sweep(oracle_mod, sc)
    for r in range(sc.world):
        st = gpu.digests[-1][r]["states"]
        assert (st["log_start_offset"] > 0).all(), (r, st["log_start_offset"])  # every ring wrapped
        assert gpu.counters[-1][r][1:3] == (0, 0) and gpu.counters[-1][r][0] == 5 * X.PARTS_I * X.NREC_I
    caught_up(sc, gpu)


@pytest.mark.parametrize("fld", X.FIELDS)
def test_flips_by_field(oracle_mod, fld):
    # B: one flipped byte per round in the named field of a record of each length that has it; the
    # entry refused in a round catches up in the region that carries the next flip
    sc = X.scenario_b(fld)
    ora, gpu = sweep(oracle_mod, sc)
    n = len(X.b_lengths(fld))
    assert [len(f) for f in gpu.flips] == [1] * n + [0]
    # one CRC refusal of one entry per flip, each sent again as one catch-up entry
    assert gpu.counters[-1][1][1:3] == (n, 0) and gpu.counters[-1][0][4] == n, gpu.counters[-1]
    assert gpu.counters[-1][0][1:3] == (0, 0)
    caught_up(sc, gpu)


def test_flips_by_place(oracle_mod):
    # B: table indices 63 and 64, an entry's first and last record, the gap part of a catch-up entry,
    # a record over 4 KB, and the entry-index word of a consumer-offset row (structural: all 4 entries)
    sc = X.scenario_b_places()
    _, gpu = sweep(oracle_mod, sc)
    assert [c[1][1] for c in gpu.counters] == [1, 2, 3, 4, 5, 6, 10, 10], [c[1] for c in gpu.counters]
    assert gpu.counters[-1][1][2] == 0 and gpu.counters[-1][0][4] == 10
    caught_up(sc, gpu)


def test_two_slots_on_one_follower(oracle_mod, verify_grid):
    # B2: world 2, RF 3: a refusal of either local slot refuses both, counted once; nothing reaches
    # either ring (the digests hold both rings whole). 760 records a region are 12 verify tasks, so
    # with one workgroup its waves take a second task each
    sc = X.scenario_b2()
    ora, gpu = sweep(oracle_mod, sc)
    assert [c[1][1] for c in gpu.counters] == [1, 2, 2] and [c[0][4] for c in gpu.counters] == [0, 2, 4]
    assert ora.refused[0][(0, 1)] == [0, 1] and ora.refused[1][(0, 1)] == [2, 3]
    caught_up(sc, gpu)


def test_two_sources_one_follower(oracle_mod, verify_grid):
    # B3: world 3, RF 3: ranks 0 and 1 both send rank 2 a flipped region in round 1, a 17-byte record
    # in one and a 4097-byte record in the other; each source loses exactly that entry (two regions of
    # 6 or 8 tasks each: with one workgroup a wave's second task lies in the other source's region)
    sc = X.scenario_b3()
    ora, gpu = sweep(oracle_mod, sc)
    assert {sd: e for sd, e in ora.refused[1].items() if e} == {(0, 2): [0], (1, 2): [2]}
    assert [c[1] for c in gpu.counters[-1]] == [0, 0, 2] and [c[4] for c in gpu.counters[-1]] == [1, 1, 0]
    caught_up(sc, gpu)


def test_copy_edges(oracle_mod):
    # C: entries of n x 16 KiB and 16 bytes either side at each of the copy's 8 line phases, 64 KiB
    # rings wrapping inside a chunk
    sc = X.scenario_c()
    _, gpu = sweep(oracle_mod, sc)
    st = gpu.digests[-1][0]["states"]
    assert (st["log_end_pos"] > sc.cfg["segment_bytes"]).all() and gpu.counters[-1][0][1:3] == (0, 0)
    caught_up(sc, gpu)


def test_task_edges(oracle_mod, verify_grid):
    # D: two sources per follower, 1 to 129 records per region, records over 1 KB at lanes 63 and 0
    sc = X.scenario_d()
    _, gpu = sweep(oracle_mod, sc)
    assert all(c[0] == 2 * sum(X.D_COUNTS) and c[1:3] == (0, 0) for c in gpu.counters[-1]), gpu.counters[-1]
    caught_up(sc, gpu)
