"""Stage 3's two load rounds against the CPU oracle, bit for bit: what the issue
order newly exposes beside the sweeps of tests/test_gpu_append_device.py.

Round 1 loads a task's record words through bounds-checked views of its batch (pidx, len,
payload_off) next to the engine's scratch on clamped indices, the batch's verdict and the nibble and
pad tables; round 2 the partition words and the payload. So: launch groups that mix packed and
explicit-offset batches and batches of 0, 1, 33 and 1025 records; task counts that leave waves of a
workgroup without a task (they still copy tables and take both barriers), in the 256-thread kernel
and in the 512-thread kernel of an engine with a transport; the pad constants on the image, piecewise
and large-record paths, with and without a rejected batch in the same group; and all of it again on
the looping path (RMQ_WG3_ALL=0) and with per-pair payload loads (RMQ_S3_STAGE=0).

16 partitions, RF 3, launch groups of 4. Every batch is compared with the oracle given the same
arrays: out offsets, stats, state, every replica's whole ring, the index.
"""
import numpy as np
import pytest

import device_batch_util as D
from parity import compare_state
from repl_sim import exchange_round, notice_round, place, rank_cfg
from ripplemq_amd.engine import Engine, EngineConfig, LocalHub
from ripplemq_amd.sharding import rank_view
from ripplemq_amd.workload import Batch

pytestmark = pytest.mark.gpu

P = 16
KNOBS = [None, "RMQ_S3_STAGE", "RMQ_WG3_ALL"]  # None: the default path; else the knob set to 0
KNOB_IDS = ["default", "stage0", "wg3all0"]


def _rng(tag: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[0x53335232, tag]))  # "S3R2"


def packed(name: str, lens, tag: int, **kw) -> D.Case:
    lens = np.asarray(lens, np.uint32)
    n = len(lens)
    b = Batch(((np.arange(n) * 5 + tag) % P).astype(np.uint32), lens,
              _rng(tag).integers(0, 256, int(lens.sum()), dtype=np.uint8))
    return D.Case(name, b, **kw)


def explicit(name: str, lens, tag: int) -> D.Case:
    """Explicit payload offsets: record k starts k % 7 bytes after the end of the one before it."""
    lens = np.asarray(lens, np.uint32)
    n = len(lens)
    offs, cur = [], 0
    for k, L in enumerate(lens.tolist()):
        cur += k % 7
        offs.append(cur)
        cur += L
    b = Batch(((np.arange(n) * 3 + tag) % P).astype(np.uint32), lens,
              _rng(tag).integers(0, 256, max(cur, 1), dtype=np.uint8))
    return D.Case(name, b, np.array(offs, np.uint64))


def rejected(tag: int) -> D.Case:
    """A packed batch whose payload_bytes is one short of sum(len): stage 2 rejects all of it."""
    c = packed("rejected", [40] * 70, tag)
    c.declared, c.invalid = 40 * 70 - 1, True
    return c


PAD_LENS = (0, 1, 15, 16, 17, 112, 113, 1024, 1025, 4097)


def pad_lens():
    """Every pad 0..15 on the image path (at most 112 B), the piecewise path (113 B..1 KB) and in
    the large-record waves (over 1 KB), the listed boundary lengths first."""
    img = [L for L in PAD_LENS if L <= 112] + list(range(97, 112))
    piece = [113, 1024] + list(range(114, 129))
    big = [1025, 4097] + list(range(1026, 1041))
    return img + piece + big


@pytest.fixture
def pair(oracle_mod, monkeypatch):
    made = []

    def make(knob=None, **kw):
        if knob:
            monkeypatch.setenv(knob, "0")
        cfg = D.small_config(num_partitions=P, pipeline_depth=4, **kw)
        dev, ora = Engine(cfg), oracle_mod.OracleEngine(cfg)
        made.extend([dev, ora])
        return cfg, dev, ora

    yield make
    for e in made:
        e.close()


def run_group(cfg, dev, ora, cases, shifts=(0, 4, 8, 12)):
    """The cases as device batches submitted back to back (one launch group of up to 4), each
    checked against the oracle in order, then state, whole rings and index."""
    dbs = [D.device_case(dev, c, shifts[k % len(shifts)]) for k, c in enumerate(cases)]
    tickets = [db.submit() for db in dbs]
    stats = [D.check_ticket(dev, ora, db, t, c.invalid, f"{c.name} at {k}")
             for k, (db, t, c) in enumerate(zip(dbs, tickets, cases))]
    compare_state(dev, ora, cfg, full_rings=True)
    for db in dbs:
        db.free()
    return stats


# ---- a. mixed payload forms and batch sizes in one launch group
@pytest.mark.parametrize("knob", KNOBS, ids=KNOB_IDS)
def test_mixed_payload_forms_in_one_group(pair, knob):
    cfg, dev, ora = pair(knob)
    mixed = [packed("packed-a", [100] * 70, 1), explicit("explicit-a", [90, 7, 0, 130] * 12, 2),
             packed("packed-b", [17, 112, 113, 0] * 10, 3), explicit("explicit-b", [100] * 33, 4)]
    sizes = [packed("n0", [], 5), packed("n1", [77], 6), explicit("n33", [60] * 33, 7), packed("n1025", [24] * 1025, 8)]
    for rnd in range(2):  # (the second pass lands on rings the first one filled)
        for cases in (mixed, sizes):
            stats = run_group(cfg, dev, ora, cases, shifts=(4 * rnd, 4, 8, 12))
            assert [s["appended"] for s in stats] == [c.batch.n for c in cases]


# ---- b. task counts that are no multiple of the workgroup's waves
@pytest.mark.parametrize("knob", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("n", [33, 65])
def test_waves_without_a_task(pair, n, knob):
    # 2 and 3 tasks in workgroups of 4 waves: the others copy their table blocks and take both barriers
    cfg, dev, ora = pair(knob)
    for rnd in range(2):
        (sd,) = run_group(cfg, dev, ora, [packed(f"alone-{n}", [100] * n, 10 + n + rnd)], shifts=(4 * rnd,))
        assert sd["appended"] == n


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


@pytest.mark.parametrize("n", [33, 65])
def test_waves_without_a_task_transport_kernel(oracle_mod, n):
    # the same through the kernel of an engine with a transport (512 threads: 8 waves, 2 or 3 tasks),
    # two ranks on the in-process hub, RF 3: every round is one batch of n records alone
    world, rf, ppr, rounds = 2, 3, P // 2, 2
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=1 << 16, index_interval=256,
                        max_batch_records=4096, max_batch_bytes=1 << 20, pipeline_depth=1)
    views = [rank_view(r, world, ppr, rf) for r in range(world)]
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    batches = [[packed(f"x{r}{k}", [100] * n, 40 + 10 * r + k).batch
                for k in range(rounds)] for r in range(world)]
    for r in range(world):
        for b in batches[r]:
            b.pidx %= views[r].led  # a rank appends to the partitions it leads (local indices)
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
                oras[r].append(b.pidx, b.lens, b.payload)
            exchange_round(oras)
        notice_round(oras)
        for r in range(world):
            st = engs[r].replication_stats()
            assert st["rounds"] == rounds and st["refused_crc"] == 0 and st["refused_log"] == 0, st

            def local_slots(p, r=r):
                return [s for s in range(rf) if views[r].ranks[p][s] == r]
            compare_state(engs[r], oras[r], cfgs[r], local_slots=local_slots, full_rings=True)
        assert sum(oras[r].state(p)["log_end_offset"] for r in range(world) for p in range(views[r].led)) == world * rounds * n
    finally:
        for o in oras:
            o.close()
        for e in engs:
            e.close()
        hub.close()


# ---- c. pad constants on every path
@pytest.mark.parametrize("knob", KNOBS, ids=KNOB_IDS)
def test_pad_constants_on_every_path(pair, knob):
    # one batch alone, then the same lengths beside a rejected batch of the same group (its verdict
    # is read in round 1 with the record words; the pad tables came in with the same round)
    cfg, dev, ora = pair(knob, segment_bytes=1 << 20)
    lens = pad_lens()
    assert set(PAD_LENS) <= set(lens) and {(-L) % 16 for L in lens if L > 1024} == set(range(16))
    (sd,) = run_group(cfg, dev, ora, [packed("pads", lens, 20)])
    assert sd["appended"] == len(lens)
    for where in (0, 2):
        cases = [packed("pads-a", lens, 21 + where), explicit("pads-b", lens[::-1], 22 + where)]
        cases.insert(where, rejected(23 + where))
        stats = run_group(cfg, dev, ora, cases)
        assert [s["rejected_invalid"] for s in stats] == [c.batch.n if c.invalid else 0 for c in cases]
        assert [s["appended"] for s in stats] == [0 if c.invalid else c.batch.n for c in cases]
