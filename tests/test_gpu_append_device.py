"""Device-memory appends (RMQ_MEM_DEVICE, what bench.py measures) against the CPU oracle, bit for bit.

Every case puts a batch in device memory with tests/device_batch_util.py (payload at a chosen residue
or address, every named byte range inside the allocation, 0xFF around the payload), appends it with
Engine.append_device and compares out offsets, stats, state, whole rings, index and consumer offsets
with the oracle after every batch. tests/test_append_edges_model.py proves on the CPU which stage-3
classes each table holds.
"""
import pytest

import device_batch_util as D
from parity import compare_state
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import Engine, EngineError

pytestmark = pytest.mark.gpu


@pytest.fixture
def pair(oracle_mod):
    made = []

    def make(**kw):
        cfg = D.small_config(**kw)
        dev, ora = Engine(cfg), oracle_mod.OracleEngine(cfg)
        made.extend([dev, ora])
        return cfg, dev, ora

    yield make
    for e in made:
        e.close()


def run_case(cfg, dev, ora, case, shift=0, **kw):
    db = D.device_case(dev, case, shift, **kw)
    what = f"{case.name} shift {shift}"
    sd = D.append_device_checked(dev, ora, db, case.invalid, what)
    try:
        compare_state(dev, ora, cfg, full_rings=True)
    except AssertionError as ex:
        raise AssertionError(f"{what}: {ex}") from None
    db.free()
    return sd


# ---- a. length x residue
@pytest.mark.parametrize("order", D.ORDERS)
@pytest.mark.parametrize("make", [D.explicit_table, D.packed_table], ids=["explicit", "packed"])
def test_lengths_at_every_residue(pair, make, order):
    # 22 lengths at the 7 / 8 piece, 8 / 9 piece (kPR) and 64 / 65 piece (kBigPieces) edges, each at all
    # 16 start residues, the payload base at residue 0, 4, 8 and 12; sorted: tasks of one length,
    # permuted: mixed tasks. Twice over: the second pass lands on rings that wrap (retention, pieces
    # a later piece of the same group overwrites).
    cfg, dev, ora = pair()
    case = make(order)
    for shift in D.SHIFTS + D.SHIFTS:
        sd = run_case(cfg, dev, ora, case, shift)
        assert sd["appended"] == case.batch.n
    assert max(ora.state(p)["log_start_offset"] for p in range(D.P)) > 0, "the rings must wrap"


# ---- b. span and tail edges
def test_span_edges(pair):
    # a staged span of exactly 256 blocks, 257 by a 4-byte shift and by one more byte, an empty span
    cfg, dev, ora = pair()
    for case, shift in D.span_cases():
        assert case.expect <= D.classes(case.batch, shift)
        sd = run_case(cfg, dev, ora, case, shift)
        assert sd["appended"] == case.batch.n


@pytest.mark.parametrize("n", D.TAIL_COUNTS)
def test_task_and_tile_tails(pair, n):
    # n % 32 and n % 1024 tails; payload_bytes is the exact payload size and 0xFF follows the last
    # declared byte, so a span read past the end that reached a ring would show
    cfg, dev, ora = pair()
    case = D.tail_case(n)
    for shift in (0, 12):
        sd = run_case(cfg, dev, ora, case, shift)
        assert sd["appended"] == n


# ---- c. range check, explicit offsets
@pytest.mark.parametrize("rank", ["sort", "hash"])
def test_range_check_explicit_offsets(pair, monkeypatch, rank):
    # o + L == D, (o == D, L == 0), (o == D + 1, L == 0) are valid; one record one byte over rejects
    # the whole batch (rejected_invalid == n, nothing written), wherever it sits: tile 0, tile 1, on a
    # record of an unknown partition. The engine goes on as if the batch had not been sent. hash: the
    # same rule in stage 1 without a sort (RMQ_RANK=1, stage1_tile_hash has a check of its own).
    if rank == "hash":
        monkeypatch.setenv("RMQ_RANK", "1")
    cfg, dev, ora = pair()
    valid = D.explicit_range_case()
    sd = run_case(cfg, dev, ora, valid)
    assert sd["appended"] == valid.batch.n - 1 and sd["rejected_no_partition"] == 1
    for kind in D.RANGE_KINDS:
        for place in D.RANGE_PLACES:
            sd = run_case(cfg, dev, ora, D.explicit_range_case(kind, place), shift=4)
            assert sd["rejected_invalid"] == valid.batch.n
    sd = run_case(cfg, dev, ora, valid, shift=8)
    assert sd["appended"] == valid.batch.n - 1


# ---- d. range check, packed
@pytest.mark.parametrize("n", [33, D.RANGE_N])
def test_range_check_packed(pair, n):
    # sum(len) == payload_bytes is valid, sum(len) == payload_bytes + 1 rejects the batch
    cfg, dev, ora = pair()
    for over in (0, 1, 0):
        sd = run_case(cfg, dev, ora, D.packed_range_case(n, over), shift=4 * over)
        assert sd["appended"] == (0 if over else n) and sd["rejected_invalid"] == (n if over else 0)


# ---- e. range check inside a launch group
@pytest.mark.parametrize("where", [0, 1, 3])
def test_invalid_batch_inside_a_launch_group(pair, where):
    # four device batches back to back (one launch group of pipeline_depth 4), one of them invalid:
    # the other three apply, their offsets continue as if it were absent, state and whole rings
    # equal the oracle that saw only the three
    cfg, dev, ora = pair(pipeline_depth=4)
    good = [D.tail_case(64), D.mixed40(), D.explicit_range_case()]
    bad = D.packed_range_case(D.RANGE_N, 1) if where != 1 else D.explicit_range_case("end_plus_1", "tile1")
    for rnd in range(2):  # (the second group lands on rings the first one filled)
        cases = list(good)
        cases.insert(where, bad)
        dbs = [D.device_case(dev, c, 4 * ((k + rnd) % 4)) for k, c in enumerate(cases)]
        tickets = [db.submit() for db in dbs]
        stats = [D.check_ticket(dev, ora, db, t, c.invalid, f"{c.name} at {k}")
                 for k, (db, t, c) in enumerate(zip(dbs, tickets, cases))]
        assert [s["rejected_invalid"] for s in stats] == [c.batch.n if c.invalid else 0 for c in cases]
        assert sum(s["appended"] for s in stats) == sum(c.batch.n for c in good) - 1
        compare_state(dev, ora, cfg, full_rings=True)
        for db in dbs:
            db.free()


# ---- f. the pinned path: the same device check
def test_range_check_pinned(pair):
    cfg, dev, ora = pair()
    cases = [D.explicit_range_case()]
    cases += [D.explicit_range_case(k, p) for k in D.RANGE_KINDS for p in D.RANGE_PLACES]
    cases += [D.packed_range_case(n, over) for n in (33, D.RANGE_N) for over in (0, 1)]
    cases += [D.explicit_range_case()]
    for case in cases:
        sd = D.append_pinned_checked(dev, ora, case)
        assert bool(sd["rejected_invalid"]) == case.invalid
        compare_state(dev, ora, cfg, full_rings=True)


# ---- g. payload addresses around a multiple of 2^31
def test_payload_addresses_around_2g(pair):
    # one untouched allocation of 2 GiB + 1 MiB holds a multiple B of 2^31: payloads straddling B,
    # wholly above and wholly below it (one side of B has bit 31 set; a B that is a multiple of 2^32
    # makes the straddle carry into the address's high word)
    cfg, dev, ora = pair()
    size = (2 << 30) + (1 << 20)
    try:
        lo = dev.device_alloc(size)
    except EngineError as ex:
        if ex.status == A.RMQ_ENOMEM:
            pytest.skip("no 2 GiB of device memory to place payloads in")
        raise
    try:
        B = (lo + (1 << 31) - 1) & ~((1 << 31) - 1)
        if B - lo < (128 << 10):
            B += 1 << 31  # (still inside: at least 896 KiB follow it)
        assert lo + (128 << 10) <= B <= lo + size - (128 << 10)
        cases = [D.tail_case(64), D.mixed40()]
        for case in cases:
            half = (case.batch.payload.size // 2) & ~15
            for name, at in (("straddle", B - half), ("above", B + 4096), ("below", B - (64 << 10))):
                for shift in (0, 12):
                    db = D.device_case(dev, case, shift, margin=4096, at=at, region=(lo, lo + size))
                    end = db.payload_addr + case.batch.payload.size
                    assert {"straddle": db.payload_addr < B < end, "above": db.payload_addr >= B,
                            "below": end <= B}[name]
                    D.append_device_checked(dev, ora, db, False, f"{case.name} {name} B={B:#x} shift {shift}")
                    compare_state(dev, ora, cfg, full_rings=True)
                    db.free()
    finally:
        dev.sync()
        dev.device_free(lo)
