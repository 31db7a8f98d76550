"""Stage 1 on the device (pipeline.hip: stage1_tile, stage1_tile_hash) at its tile, slot, wave and
key-width edges: the case tables of tests/stage1_edges_util.py through the HIP engine and the C
oracle (out offsets, stats, state, rings, live index entries and a fetch of every touched partition,
bit for bit). tests/test_stage1_edges_model.py proves without a GPU that each table holds the edge it
is named for, in both kernel geometries, and that the oracle agrees with the model of stage 1.

Every table runs with the sort (RMQ_RANK unset) and with the hash counters (RMQ_RANK=1), through the
256-thread kernel of an engine alone and through the 512-thread kernel of an engine with a
replication transport; `runs` and `nin` also with one stage-1 workgroup ranking every tile in turn
(RMQ_S1_WGS=1) and with tiles taken from the group's counter (RMQ_STEAL=1). The batches of a group
are submitted before any is waited for.

The transport run: two ranks on the in-process hub, RF 2; rank 0 leads every partition with its
follower on rank 1, so its launches are the transport kernel's and its engine has exactly the
table's P partitions; rank 1 submits a batch without records for each of rank 0's. Both ranks'
logs are compared. P = 65536 runs on it as on the engine alone: nothing had to be made smaller.

No 64 partitions of the 65536 an engine may have share a first hash slot (34 at most): the `hash`
table's crowded input slots hold 64 leaders over two neighbouring first slots, 34 and 32 on one.

On an MI355X the file's 52 cases took 9 s in all; the slowest, the P = 65536 tables on the
transport, 0.6 to 0.8 s each, on an engine alone 0.13 to 0.25 s (creating that engine takes 0.02 s,
so every case creates its own). The P = 65536 engine alone takes 472 MiB of device memory by the
driver's count, 710 MiB with the transport run's two replica slots (stage1_edges_util.big_cfg).

With one line of stage 1 changed on purpose (a build kept out of the repository), these tables
fail where the random streams of test_gpu_parity.py need not: a hash leader that loses the CAS to
another key and stays on its slot fails keys-P1024, keys-P65536 and hash in hash mode on both
kernels while test_variant_modes_small and test_multi_pass_sort pass; `hb[r] = head` and a `cin`
loop that looks one wave back fail every sort-mode table but keys-P1 / hash respectively."""
import threading

import numpy as np
import pytest

import device_batch_util as D
import stage1_edges_util as U
from parity import compare_state, run_ops
from repl_sim import exchange_round, notice_round, place
from ripplemq_amd.engine import Engine, EngineConfig, LocalHub
from ripplemq_amd.sharding import RankView

pytestmark = pytest.mark.gpu

MODES = {"sort": {}, "hash": {"RMQ_RANK": "1"}}
KNOBS = {"s1wgs1": {"RMQ_S1_WGS": "1"}, "steal": {"RMQ_STEAL": "1"}}
FULL_RINGS_P = 300   # whole rings up to this many partitions, the retained windows of a subset above
FETCH_RECORDS = 64


def submit(dev, c):
    """One case's batch: packed from ordinary host arrays; with explicit offsets from page-locked
    arrays (their ranges are checked on the device, by stage 1) that hold every byte range the case
    names. Returns (ticket, out offsets, the arrays the oracle gets)."""
    b = c.batch
    if c.poff is None:
        t, out = dev.append_async(b.pidx, b.lens, b.payload)
        return t, out, (b.pidx, b.lens, b.payload, None)
    n, declared = b.n, U.declared_bytes(c)
    ends = D.record_starts(b, c.poff) + b.lens.astype(np.int64)
    size = max(b.payload.size, declared, int(ends.max(initial=0))) + 16
    pidx, lens, out = dev.host_empty(n, np.uint32), dev.host_empty(n, np.uint32), dev.host_empty(n, np.uint64)
    pay, poff = dev.host_empty(size, np.uint8), dev.host_empty(n, np.uint64)
    pidx[:], lens[:], out[:], pay[:], poff[:] = b.pidx, b.lens, D.OUT_UNWRITTEN, 0xFF, c.poff
    pay[:b.payload.size] = b.payload
    t = dev.append_pinned_async(pidx, lens, pay, out, payload_off=poff, payload_bytes=declared)
    return t, out, (b.pidx, b.lens, np.array(pay[:declared]), c.poff)


def check_group(dev, ora, group, subs, what):
    stats = []
    for c, (tk, out, arrays) in zip(group, subs):
        sd = dev.wait(tk)
        assert sd is not None, f"{what} {c.name}: the ticket is still pending"
        D.check_result(ora, arrays, sd, np.array(out), c.invalid, f"{what} batch {c.name}")
        stats.append(sd)
    return stats


def checked_parts(t):
    """Every touched partition where rings are compared whole, else the engine's first and last
    partitions, the table's extremes and every eighth touched one."""
    parts = U.touched(t)
    if t.P <= FULL_RINGS_P:
        return list(range(t.P))
    keep = set(t.notes.get("ext", ())) | {0, 1, t.P - 2, t.P - 1} | set(parts[::8])
    return sorted(keep)


def compare_all_states(dev, ora):
    sd, so = dev.states(), ora.states()
    if not np.array_equal(sd, so):
        bad = [i for i in range(len(sd)) if sd[i].tobytes() != so[i].tobytes()]
        raise AssertionError(f"{len(bad)} partition states differ, first {bad[0]}\n gpu={dev.state(bad[0])}\n "
                             f"cpu={ora.state(bad[0])}")


def fetch_touched(dev, ora, cfg, t, consumers=(0, 1)):
    """Every touched partition from offset 0 (consumer 0) and from its first retained offset
    (consumer 1): results and fetched bytes against the oracle."""
    pp = np.array(U.touched(t), np.uint32)
    n = len(pp)
    if 1 in consumers:
        starts = [ora.state(int(p))["log_start_offset"] for p in pp]
        for e in (dev, ora):
            e.commit_consumer_offset(pp, np.ones(n, np.uint32), starts)
    run_ops(dev, ora, cfg, [("fetch", pp, np.full(n, k, np.uint32), np.full(n, FETCH_RECORDS, np.uint32))
                            for k in consumers], check=False)


def expected_counts(t):
    cases = t.cases()
    flagged = sum(int((U.record_flags(c, t.P)[0] == U.FL_NOPART).sum()) for c in cases if not c.invalid)
    invalid = sum(c.batch.n for c in cases if c.invalid)
    return sum(c.batch.n for c in cases) - flagged - invalid, flagged, invalid


def check_counts(t, stats):
    appended, flagged, invalid = expected_counts(t)
    assert sum(s["appended"] for s in stats) == appended > 0
    assert sum(s["rejected_no_partition"] for s in stats) == flagged
    assert sum(s["rejected_invalid"] for s in stats) == invalid
    assert sum(s["rejected_no_space"] + s["rejected_not_leader"] for s in stats) == 0


def run_alone(O, t):
    cfg = EngineConfig(**t.cfg)
    full = t.P <= FULL_RINGS_P
    parts = checked_parts(t)
    stats = []
    with Engine(cfg) as dev, O.OracleEngine(cfg) as ora:
        for gi, g in enumerate(t.groups):
            what = f"{t.name} group {gi}"
            try:
                stats += check_group(dev, ora, g, [submit(dev, c) for c in g], what)
                if not full:
                    compare_all_states(dev, ora)
                compare_state(dev, ora, cfg, parts=parts, full_rings=full)
            except AssertionError as ex:
                raise AssertionError(f"{what}: {ex}") from ex
        fetch_touched(dev, ora, cfg, t)
    check_counts(t, stats)


def _run_ranks(world, body):
    errs = [None] * world

    def wrap(r):
        try:
            body(r)
        except BaseException as ex:  # noqa: BLE001 - reported below
            errs[r] = ex

    ts = [threading.Thread(target=wrap, args=(r,), daemon=True) for r in range(world)]
    for th in ts:
        th.start()
    for th in ts:
        th.join(120)
        assert not th.is_alive(), "a rank hung"
    for r, ex in enumerate(errs):
        if ex is not None:
            raise AssertionError(f"rank {r}: {ex!r}") from ex


def run_with_transport(O, t):
    world, rf, P = 2, 2, t.P
    cfgs = [EngineConfig(**{**t.cfg, "replication_factor": rf, "rank": r}) for r in range(world)]
    ranks = np.tile(np.array([0, 1], np.uint32), (P, 1))
    views = [RankView(r, np.arange(P, dtype=np.uint64), ranks, np.zeros(P, np.uint32), P if r == 0 else 0)
             for r in range(world)]
    none = np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    full = P <= FULL_RINGS_P
    parts = checked_parts(t)
    subs = []
    hub = LocalHub(world)
    engs = [Engine(c) for c in cfgs]
    oras = []
    try:
        def body(r):
            e = engs[r]
            e.attach_local(hub)
            place(e, views[r])
            for g in t.groups:  # a group is one round: closed by its size or by the sync
                if r == 0:
                    subs.append([submit(e, c) for c in g])
                else:
                    for _ in g:
                        e.append_async(*none)
                e.sync()

        _run_ranks(world, body)
        oras = [O.OracleEngine(c) for c in cfgs]
        for r in range(world):
            place(oras[r], views[r], world)
        stats = []
        for gi, g in enumerate(t.groups):
            stats += check_group(engs[0], oras[0], g, subs[gi], f"{t.name} group {gi}")
            exchange_round(oras)
            notice_round(oras)
        check_counts(t, stats)
        st = [e.replication_stats() for e in engs]
        assert st[0]["out_entries"] == P and st[1]["in_entries"] == P  # rank 0's launches fill an outbox
        for s in st:
            assert s["rounds"] == len(t.groups) and s["refused_crc"] == 0 and s["refused_log"] == 0, s
        assert st[1]["records_ingested"] == sum(s["appended"] for s in stats)
        for r in range(world):
            if not full:
                compare_all_states(engs[r], oras[r])
            compare_state(engs[r], oras[r], cfgs[r], parts=parts, full_rings=full, local_slots=lambda p, r=r: [r])
        fetch_touched(engs[0], oras[0], cfgs[0], t, consumers=(0,))
    finally:
        for o in oras:
            o.close()
        for e in engs:
            e.close()
        hub.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", U.TABLES)
def test_engine_alone(oracle_mod, monkeypatch, name, mode):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    run_alone(oracle_mod, U.table(name))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", U.TABLES)
def test_engine_with_transport(oracle_mod, monkeypatch, name, mode):
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    run_with_transport(oracle_mod, U.table(name))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("name", U.POSITIONAL)
def test_workgroup_knobs(oracle_mod, monkeypatch, name, knob, mode):
    """One workgroup ranks every tile of a group in turn, reusing its LDS from tile to tile; with
    RMQ_STEAL the tiles come from the group's counter and stage-3 workgroups rank some of them."""
    for k, v in {**MODES[mode], **KNOBS[knob]}.items():
        monkeypatch.setenv(k, v)
    run_alone(oracle_mod, U.table(name))
