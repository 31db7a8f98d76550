"""Ring moves (rmq_set_segments: migrate_kernel in csrc/control.hip and its host half) against the CPU
oracle, bit for bit: moves of more than one chunk on data, into a block an earlier log dirtied,
mixed items in one call, the edges of a shrink's retention, fetches, held fetch tickets and
batches in flight around a move, refused calls, and a follower whose ring differs from its
leader's. The scenarios and their guards come from tests/ring_move_util.py (the guards run here again
on the oracle of the pair; tests/test_oracle_ring_moves.py runs them without a GPU). After every
move the state, every byte of every replica ring, the live index entries and the consumer offsets
equal the oracle's (parity.compare_state, full rings), and every slot of a moved partition's index
ring holds its live entry or zero (parity.compare_index_slots)."""
import threading

import numpy as np
import pytest

import ring_move_util as U
import scrub_util
from parity import compare_index_slots, compare_state
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine, LocalHub

pytestmark = pytest.mark.gpu

KiB = U.KiB


def run(oracle_mod, scn, after=None):
    with Engine(scn.cfg) as dev, oracle_mod.OracleEngine(scn.cfg) as ora:
        return U.play(scn, ora, dev, after)


@pytest.mark.parametrize("new_seg", [512 * KiB, 1 << 20])
def test_multi_chunk_grow_on_data(oracle_mod, new_seg):
    scn = U.multi_chunk_grow(new_seg)
    cfg = scn.cfg
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        U.play(scn, ora, dev)
        rows = dev.scrub()
        assert dev.last_scrub_rc == A.RMQ_OK
        scrub_util.assert_clean(rows, dev, cfg)
        # the whole retained log of a moved partition, verified on the device and not
        p = scn.facts["grown"][0]
        st = ora.state(p)
        pp, cc = np.array([p], np.uint32), np.zeros(1, np.uint32)
        for e in (dev, ora):
            e.commit_consumer_offset(pp, cc, np.array([st["log_start_offset"]], np.uint64))
        mx = np.array([1 << 30], np.uint32)
        plain, checked, want = dev.fetch(pp, cc, mx), dev.fetch(pp, cc, mx, verify=True), ora.fetch(pp, cc, mx)
        assert int(want[1]["count"][0]) == st["log_end_offset"] - st["log_start_offset"] > 0
        for got in (plain, checked):
            assert got[0] == want[0] and got[3] == want[3]
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_dirty_block_reuse(oracle_mod):
    run(oracle_mod, U.dirty_block_reuse())


def test_mixed_items_in_one_call(oracle_mod):
    run(oracle_mod, U.mixed_items())


@pytest.mark.parametrize("new_seg", [1 * KiB, 2 * KiB, 4 * KiB, 8 * KiB])
def test_shrink_edges(oracle_mod, new_seg):
    run(oracle_mod, U.shrink_edges(new_seg))


def test_shrink_misc(oracle_mod):
    scn = U.shrink_misc()
    with Engine(scn.cfg) as dev, oracle_mod.OracleEngine(scn.cfg) as ora:
        def zeros(snaps):
            for r in range(scn.cfg.replication_factor):
                assert not dev.read_segment(r, scn.facts["long"]).any()

        U.play(scn, ora, dev, after={"move": zeros})


def test_fetch_across_moves(oracle_mod):
    run(oracle_mod, U.fetch_across_moves())


def test_held_fetch_ticket_across_a_move(oracle_mod):
    # a fetch_async that was never polled is answered from the ring as it was before the move: every
    # call that takes the engine lock issues the held fetches first
    scn = U.fetch_across_moves()
    cfg = scn.cfg
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        for b in (op[1] for op in scn.stages[0][1]):
            dev.append(b.pidx, b.lens, b.payload)
            ora.append(b.pidx, b.lens, b.payload)
        pp, cc, mx = np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.full(1, 40, np.uint32)
        rc, want, wbuf, wused = ora.fetch(pp, cc, mx)
        assert rc == A.RMQ_OK and int(want["count"][0]) == 40 and wused > 0
        tk = dev.fetch_async(pp, cc, mx, out=np.zeros(1 << 16, np.uint8))
        for e in (dev, ora):
            e.set_segments([0], [4 * cfg.index_interval])
        assert ora.state(0)["log_start_offset"] > 40, "the move must evict the held slice"
        got = dev.fetch_poll(tk, wait=True)
        assert got is not None
        grc, res, used = got
        assert (grc, used) == (rc, wused)
        assert np.array_equal(res, want) and np.array_equal(tk.out[:used], wbuf[:wused])
        compare_state(dev, ora, cfg, full_rings=True)
        compare_index_slots(dev, ora, cfg, 0)


@pytest.mark.parametrize("depth,late", [(2, False), (3, False), (3, True)])
def test_moves_with_batches_in_flight(oracle_mod, depth, late):
    scn = U.pipelined_moves(depth, late)
    cfg = scn.cfg
    stages = dict(scn.stages)
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        subs = []
        for name in ("before", "move", "after"):  # no sync anywhere: the call drains what is in flight
            for op in stages[name]:
                if op[0] == "append":
                    b = op[1]
                    subs.append((b, dev.append_async(b.pidx, b.lens, b.payload)))
                else:
                    dev.set_segments(op[1], op[2])
        snaps = {}
        for name in ("before", "move", "after"):
            for op in stages[name]:
                if op[0] == "append":
                    b, (t, out) = subs.pop(0)
                    assert b is op[1]
                    sd = dev.wait(t)
                    oo, so = ora.append(b.pidx, b.lens, b.payload)
                    assert sd == so, f"append stats gpu={sd} cpu={so}"
                    assert np.array_equal(out, oo), "out offsets differ"
                else:
                    ora.set_segments(op[1], op[2])
            snaps[name] = [ora.state(p) for p in range(cfg.num_partitions)]
            scn.guards.get(name, lambda *a: None)(scn, snaps, ora)
        compare_state(dev, ora, cfg, full_rings=True)


def test_refused_calls_change_nothing(oracle_mod):
    scn = U.refused_calls()
    cfg = scn.cfg
    P, RF = cfg.num_partitions, cfg.replication_factor
    with Engine(cfg) as dev, oracle_mod.OracleEngine(cfg) as ora:
        def everything(e):
            icap = [U.index_capacity(cfg, e.state(p)["segment_bytes"]) for p in range(P)]
            return ([e.state(p) for p in range(P)], [e.read_segment(r, p).tobytes() for p in range(P) for r in range(RF)],
                    [e.consumer_offsets(p).tobytes() for p in range(P)],
                    [e.read_index(p, 0, icap[p]).tobytes() for p in range(P)] if e is dev else None)

        def refuse(snaps):
            before = everything(dev), everything(ora)
            for name, pidx, sizes, status, judged in scn.facts["calls"]:
                assert U.call_status(dev, pidx, sizes) == status, name
                if judged:
                    assert U.call_status(ora, pidx, sizes) == status, name
                assert (everything(dev), everything(ora)) == before, name

        # the grow after them: a call that had allocated before it refused would have taken the one
        # block it needs
        U.play(scn, ora, dev, after={"fill": refuse})


def test_follower_with_another_ring_size(oracle_mod):
    fs = U.follower_ring_script()
    world, rf = fs.world, fs.rf
    from repl_sim import place
    hub = LocalHub(world)
    engs = [Engine(c) for c in fs.cfgs]
    gate = threading.Barrier(world, timeout=60)
    errs = [None] * world
    try:
        def body(r):
            e = engs[r]
            try:
                e.attach_local(hub)
                place(e, fs.views[r])
                cut = fs.move_after * fs.group
                for b in fs.batches[r][:cut]:
                    e.append_async(b.pidx, b.lens, b.payload)
                e.sync()
                gate.wait()
                if fs.moves[r]:
                    e.set_segments(*fs.moves[r])
                gate.wait()
                for b in fs.batches[r][cut:]:
                    e.append_async(b.pidx, b.lens, b.payload)
                e.sync()
            except BaseException as ex:  # noqa: BLE001 - reported below
                errs[r] = ex
                gate.abort()

        ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
            assert not t.is_alive(), "a rank hung"
        for r, ex in enumerate(errs):
            if ex is not None:
                raise AssertionError(f"rank {r}: {ex!r}") from ex
        oras = [oracle_mod.OracleEngine(c) for c in fs.cfgs]
        try:
            U.run_follower_oracles(oras, fs)
            U.follower_guards(oras, fs)
            for r in range(world):
                st = engs[r].replication_stats()
                assert st["rounds"] == fs.rounds and st["refused_crc"] == 0 and st["refused_log"] == 0, (r, st)
                assert st["records_ingested"] == int(oras[r].counters()[0]), (r, st, oras[r].counters())

                def local_slots(p, r=r):
                    return [s for s in range(rf) if fs.views[r].ranks[p][s] == r]
                compare_state(engs[r], oras[r], fs.cfgs[r], full_rings=True, local_slots=local_slots)
            for r in range(world):
                for p in range(fs.views[r].led):
                    s = engs[r].state(p)
                    assert s["commit"] == s["log_end_offset"] > 0, (r, p, s)
        finally:
            for o in oras:
                o.close()
    finally:
        for e in engs:
            e.close()
        hub.close()
