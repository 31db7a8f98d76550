"""Stage 2's general column scan on the device (pipeline.hip: stage2_column_general, DESIGN.md
stage 2): the case tables of tests/stage2_general_util.py through the HIP engine and the C oracle
(tests/parity.py: out offsets, stats, state, rings, live index entries, fetch output, bit for bit).
tests/test_stage2_general_model.py proves without a GPU that the tables reach the scan: groups of
more than 256 tiles (A, D, E, F) or a cell of more than 2^21 - 1 units (C), and, for B and C's last
table, a batch without tiles at the end of a group whose tiles end on a chunk boundary, where the
oracle's log start differs from what a stale per-batch aggregate would give.

Batches of one group are submitted before any is waited for."""
import re

import numpy as np
import pytest

import device_batch_util as D
import stage2_general_util as U
from parity import compare_state, pipelined, run_ops
from repl_sim import exchange_round, notice_round, place, rank_cfg
from ripplemq_amd.engine import Engine, EngineConfig, LocalHub
from ripplemq_amd.sharding import rank_view

pytestmark = pytest.mark.gpu


def _run_ranks(world, body):
    import threading
    errs = [None] * world

    def wrap(r):
        try:
            body(r)
        except BaseException as ex:  # noqa: BLE001 - reported below
            errs[r] = ex

    ts = [threading.Thread(target=wrap, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
        assert not t.is_alive(), "a rank hung"
    for r, ex in enumerate(errs):
        if ex is not None:
            raise AssertionError(f"rank {r}: {ex!r}") from ex


def submit_pinned_short(dev, b):
    """The batch from page-locked arrays with payload_bytes one short of sum(len): its ranges are
    checked on the device. Returns (ticket, out offsets, the declared payload bytes)."""
    declared = b.payload.size - 1
    pidx, lens, out = dev.host_empty(b.n, np.uint32), dev.host_empty(b.n, np.uint32), dev.host_empty(b.n, np.uint64)
    pay = dev.host_empty(b.payload.size, np.uint8)
    pidx[:], lens[:], out[:], pay[:] = b.pidx, b.lens, D.OUT_UNWRITTEN, b.payload
    return dev.append_pinned_async(pidx, lens, pay, out, payload_bytes=declared), out, b.payload[:declared]


def run_group(dev, ora, batches, sync=False):
    """One "group" op: parity.pipelined, or, with a ShortBatch among them, the same with that batch
    from page-locked arrays and checked as device_batch_util.check_result checks an invalid batch."""
    if not any(isinstance(b, U.ShortBatch) for b in batches) and not sync:
        return pipelined(dev, ora, batches)
    subs = []
    for b in batches:
        if isinstance(b, U.ShortBatch):
            subs.append(submit_pinned_short(dev, b))
        else:
            subs.append(dev.append_async(b.pidx, b.lens, b.payload) + (b.payload,))
    if sync:
        dev.sync()
    stats = []
    for k, ((t, out, pay), b) in enumerate(zip(subs, batches)):
        sd = dev.wait(t)
        D.check_result(ora, (b.pidx, b.lens, pay, None), sd, np.array(out), isinstance(b, U.ShortBatch), f"batch {k}")
        stats.append(sd)
    return stats


def run_table(oracle_mod, t, full_rings=True, sync=False):
    cfg = EngineConfig(**t.cfg)
    stats = []
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        for k, op in enumerate(t.ops):
            try:
                if op[0] == "group":
                    stats += run_group(dev, ora, op[1], sync)
                    compare_state(dev, ora, cfg, full_rings=full_rings)
                else:
                    run_ops(dev, ora, cfg, [op], full_rings=full_rings)
            except AssertionError as ex:
                raise AssertionError(f"{t.name} op {k} ({op[0]}): {ex}") from ex
        fetch_from_start(dev, ora, cfg)
    assert sum(s["appended"] for s in stats), f"{t.name}: nothing was appended"
    return stats


def fetch_from_start(dev, ora, cfg, records=64):
    """Every partition from its first retained offset (consumer 1), and from offset 0 (consumer 0):
    results and fetched bytes against the oracle."""
    P = cfg.num_partitions
    pp = np.arange(P, dtype=np.uint32)
    starts = [ora.state(p)["log_start_offset"] for p in range(P)]
    for e in (dev, ora):
        e.commit_consumer_offset(pp, np.ones(P, np.uint32), starts)
    run_ops(dev, ora, cfg, [("fetch", pp, np.zeros(P, np.uint32), np.full(P, records, np.uint32)),
                            ("fetch", pp, np.ones(P, np.uint32), np.full(P, records, np.uint32))], check=False)


# ---- A: groups of more than one chunk
@pytest.mark.parametrize("name", U.A_NAMES)
def test_multi_chunk_groups(oracle_mod, name):
    t = U.table_a(name)
    stats = run_table(oracle_mod, t)
    assert sum(s["rejected_invalid"] for s in stats) == sum(b.n for b in t.batches() if isinstance(b, U.ShortBatch))
    assert sum(s["rejected_no_space"] for s in stats) == (t.notes["no_space"][2] if "no_space" in t.notes else 0)


# ---- B: a trailing empty batch on a chunk boundary, T = 512
@pytest.mark.parametrize("order", ["wait", "sync"])
def test_trailing_empty_batch_on_a_chunk_boundary(oracle_mod, order):
    """wait: each group's tickets waited for; sync: a sync after each group's submissions (the drain's
    launch replays retention from the same rows), [F] alone first."""
    t = U.table_b(order)
    run_table(oracle_mod, t, sync=order == "sync")


def test_trailing_empty_batch_read_before_any_wait(oracle_mod):
    """The [F, empty] groups and two small groups submitted, then state and a fetch from offset 0
    without a sync or a wait (late_retention_kernel reads the rows of the groups applied so far)."""
    t = U.table_b("read")
    cfg = EngineConfig(**t.cfg)
    P = cfg.num_partitions
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        for op in t.ops[:-1]:
            run_group(dev, ora, op[1])
        batches = t.ops[-1][1]
        subs = [dev.append_async(b.pidx, b.lens, b.payload) for b in batches]
        want = []
        st = [dev.state(p) for p in range(P)]
        leo = [s["log_end_offset"] for s in st]
        while [ora.state(p)["log_end_offset"] for p in range(P)] != leo:
            assert len(want) < len(batches), "device state matches no prefix of the batches"
            b = batches[len(want)]
            want.append(ora.append(b.pidx, b.lens, b.payload))
        while len(want) < len(batches) and not batches[len(want)].n:  # (an empty batch changes no state)
            b = batches[len(want)]
            want.append(ora.append(b.pidx, b.lens, b.payload))
        assert len(want) >= 4, f"only {len(want)} batches applied at the read"  # both [F, empty] groups
        assert st == [ora.state(p) for p in range(P)], f"state after {len(want)} applied batches"
        pp = np.arange(P, dtype=np.uint32)
        run_ops(dev, ora, cfg, [("fetch", pp, np.zeros(P, np.uint32), np.full(P, 64, np.uint32))], check=False)
        assert ora.state(0)["log_start_offset"] > 0
        dev.sync()
        for b in batches[len(want):]:
            want.append(ora.append(b.pidx, b.lens, b.payload))
        for k, ((tk, out), (oo, so)) in enumerate(zip(subs, want)):
            sd = dev.wait(tk)
            assert sd == so, f"batch {k}: append stats gpu={sd} cpu={so}"
            assert np.array_equal(out, oo), f"batch {k}: out offsets differ"
        compare_state(dev, ora, cfg, full_rings=True)
        fetch_from_start(dev, ora, cfg)


# ---- C: wide cells (ring windows: the rings are 64 MiB)
@pytest.mark.parametrize("name", U.C_NAMES)
def test_wide_cells(oracle_mod, name):
    t = U.table_c(name)
    stats = run_table(oracle_mod, t, full_rings=False)
    if "no_space" in t.notes:
        assert [s["rejected_no_space"] for s in stats] == [U.TILE_RECS, 0] and stats[1]["appended"] == 50
    else:
        assert all(s["appended"] == s["records"] for s in stats)


# ---- D: early group close
def test_early_group_close(oracle_mod):
    run_table(oracle_mod, U.table_d())


def test_early_group_close_launches(monkeypatch, capfd):
    """With RMQ_TRACE=1 the engine prints every pipeline launch's roles ("rmq launch <n>:
    s1 <b> batches ... | s3 <b> batches"): the three batches go through stage 1 as 2 and then 1."""
    monkeypatch.setenv("RMQ_TRACE", "1")
    t = U.table_d()
    with Engine(EngineConfig(**t.cfg)) as dev:
        capfd.readouterr()
        subs = [dev.append_async(b.pidx, b.lens, b.payload) for b in t.ops[0][1]]
        dev.sync()
        assert [dev.wait(tk)["appended"] for tk, _ in subs] == [int((b.pidx < 4).sum()) for b in t.ops[0][1]]
        lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("rmq launch")]
    roles = [tuple(int(x) for x in re.search(r"s1 (\d+) batches.*s3 (\d+) batches", ln).groups()) for ln in lines]
    assert [s1 for s1, _ in roles if s1] == [2, 1], lines
    assert sum(s3 for _, s3 in roles) == 3, lines


# ---- E: the stage-2 and stage-3 workgroup knobs over 70 partitions
@pytest.mark.parametrize("knob", [("RMQ_S2_WGS", "1"), ("RMQ_WG3_ALL", "0")], ids=["s2wgs1", "wg3all0"])
@pytest.mark.parametrize("name", U.E_NAMES)
def test_workgroup_knobs(oracle_mod, monkeypatch, name, knob):
    monkeypatch.setenv(*knob)
    run_table(oracle_mod, U.table_e(name))


# ---- F: the kernel of an engine with a transport (512 threads)
def test_transport_kernel_multi_chunk(oracle_mod):
    """Two ranks on the in-process hub, RF 3, launch groups of one batch: every round is one batch of
    300 tiles of zero-length records per rank (the 512-thread stage 2 and its outbox plan, T > 256)."""
    world, rf, ppr, rounds = U.F_WORLD, U.F_RF, U.F_PPR, U.F_ROUNDS
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=4 * U.MIB, index_interval=U.I,
                        max_batch_records=U.F_TILES * U.TILE_RECS, max_batch_bytes=1 << 20, pipeline_depth=1)
    views = [rank_view(r, world, ppr, rf) for r in range(world)]
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    batches = U.f_batches(ppr)
    assert all(v.led == ppr for v in views)
    hub = LocalHub(world)
    engs = [Engine(c) for c in cfgs]
    oras = []
    try:
        def body(r):
            e = engs[r]
            e.attach_local(hub)
            place(e, views[r])
            for b in batches[r]:
                e.append_async(b.pidx, b.lens, b.payload)
            e.sync()

        _run_ranks(world, body)
        oras = [oracle_mod.OracleEngine(c) for c in cfgs]
        for r in range(world):
            place(oras[r], views[r], world)
        for k in range(rounds):
            for r in range(world):
                b = batches[r][k]
                _, so = oras[r].append(b.pidx, b.lens, b.payload)
                assert so["appended"] == b.n
            exchange_round(oras)
        notice_round(oras)
        for r in range(world):
            st = engs[r].replication_stats()
            assert st["rounds"] == rounds and st["refused_crc"] == 0 and st["refused_log"] == 0, st

            def local_slots(p, r=r):
                return [s for s in range(rf) if views[r].ranks[p][s] == r]
            compare_state(engs[r], oras[r], cfgs[r], local_slots=local_slots, full_rings=True)
        assert sum(oras[r].state(p)["log_end_offset"] for r in range(world) for p in range(ppr)) \
            == world * rounds * batches[0][0].n
    finally:
        for o in oras:
            o.close()
        for e in engs:
            e.close()
        hub.close()
