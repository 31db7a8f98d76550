"""The case tables of tests/stage2_general_util.py without a GPU: that each holds the edge it is named
for (from the model's arithmetic alone: the launch groups and their tile0[], the cells), that the
oracle takes every batch as the table expects and agrees with the independent partition model, and
that the oracle's result on the trailing-empty-batch tables differs from what a stale per-batch
aggregate would give, so the device test of those tables cannot pass by accident."""
import functools

import numpy as np
import pytest

import partition_rules_util as R
import stage2_general_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import EngineConfig, EngineError
from ripplemq_amd.workload import Batch


@functools.lru_cache(maxsize=None)
def table(kind: str, name: str = "") -> U.Table:
    """The tables are built once for the module (tests only read them)."""
    return {"A": U.table_a, "E": U.table_e, "B": U.table_b, "C": U.table_c}[kind](name) if kind != "D" else U.table_d()


ALL = ([("A", n) for n in U.A_NAMES] + [("E", n) for n in U.E_NAMES] + [("B", o) for o in U.B_ORDERS]
       + [("C", n) for n in U.C_NAMES] + [("D", "")])
IDS = [f"{k}-{n}" if n else k for k, n in ALL]


# ---- the model's own parts --------------------------------------------------------------------

def test_cells_against_a_record_loop():
    b = U.spread(2 * U.TILE_RECS + 77, 3, 5, hi=100)
    cnt, b16 = U.cells(b, 3)
    want_c, want_b = np.zeros((3, 3), int), np.zeros((3, 3), int)
    for k, (p, n) in enumerate(zip(b.pidx.tolist(), b.lens.tolist())):
        if p < 3:
            want_c[k // 1024][p] += 1
            want_b[k // 1024][p] += R.rec_size(n) // 16
    assert (b.pidx == 3).sum() == U.UNKNOWN_TAIL and b.pidx[-1] < 3
    assert np.array_equal(cnt, want_c) and np.array_equal(b16, want_b)


def test_group_layout_rule():
    lay = lambda tiles, depth, mbr: [g.tile0 for g in U.group_layout([t * 1024 for t in tiles], depth, mbr)]
    assert U.group_tile_limit(5, 65 * 1024) == 328 and U.group_tile_limit(4, 262144) == 512
    assert U.group_tile_limit(8, 524288) == 512 and U.group_tile_limit(2, 1025) == 4
    assert lay([1, 1, 1], 2, 1024) == [[0, 1, 2], [0, 1]]              # closes at depth batches
    assert lay([200, 200, 200], 4, 200 * 1024) == [[0, 200, 400], [0, 200]]  # 400 + 200 > 512
    assert lay([256, 256, 1], 4, 262144) == [[0, 256, 512], [0, 1]]    # 512 is not past the limit
    assert lay([0, 0, 3], 3, 4096) == [[0, 0, 0, 3]]                   # empty batches take a place
    assert U.tiles_of(1) == 1 and U.tiles_of(1024) == 1 and U.tiles_of(1025) == 2 and U.tiles_of(0) == 0


def test_fast_model_is_the_partition_model():
    """FastPartitionModel against PartitionModel, record by record: every rejection kind, retention."""
    S, I, P = 4096, 256, 3
    slow, fast = R.PartitionModel(P, 2, S, I), U.FastPartitionModel(P, 2, S, I)
    g = np.random.default_rng(7)
    for k in range(30):
        n = int(g.integers(0, 90))
        pidx = g.integers(0, P + 1, n).astype(np.uint32)  # P: an unknown partition
        lens = g.integers(0, 120 if k % 5 else 400, n).astype(np.uint32)  # (every fifth: partitions over S - I)
        so, ss = slow.append(pidx, lens)
        fo, fs = fast.append(pidx, lens)
        assert ss == fs and so == fo.tolist(), k
        for p in range(P):
            assert slow.state(p) == fast.state(p), (k, p)
            assert slow.live_index(p) == fast.live_index(p), (k, p)
    assert fs and any(slow.state(p)["log_start_offset"] for p in range(P))


# ---- layout -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", ALL, ids=IDS)
def test_tables_hold_their_chunk_edges(kind, name):
    t = table(kind, name)
    groups = [g for _, g in U.expected_groups(t)]
    rel = set().union(*(U.chunk_relations(g) for g in groups))
    assert t.want <= rel, f"{t.name}: misses {t.want - rel}"
    cfg = EngineConfig(**t.cfg)
    limit = U.group_tile_limit(cfg.pipeline_depth, cfg.max_batch_records)
    assert all(g.T <= limit <= U.MAX_TILES and g.nb <= cfg.pipeline_depth for g in groups)
    assert all(b.n <= cfg.max_batch_records and b.payload.size <= cfg.max_batch_bytes for b in t.batches())
    if kind in ("A", "E", "D"):  # every table of these reaches the scan through its tile count
        assert max(g.T for g in groups) > U.CHUNK


def test_named_layouts():
    T0 = lambda kind, name: [g.tile0 for _, g in U.expected_groups(table(kind, name))][-1]
    assert T0("A", "alone-257") == [0, 257] and T0("A", "alone-512") == [0, 512]
    assert T0("A", "five-65") == [0, 65, 130, 195, 260, 325]  # 325 % 4 == 1, stride 328
    assert T0("A", "256+1") == [0, 256, 257] and T0("A", "255+2") == [0, 255, 257]
    assert T0("A", "128+128+1") == [0, 128, 256, 257] and T0("A", "100+200+100") == [0, 100, 300, 400]
    assert T0("A", "rejected-straddles") == [0, 250, 262, 272]
    assert T0("A", "no-space-straddles") == [0, 5, 305, 315]
    assert T0("A", "empty-at-256") == [0, 256, 256, 286]
    assert T0("A", "empty-at-end-300") == [0, 300, 300] and T0("A", "two-empty-at-end-300") == [0, 150, 300, 300, 300]
    # the groups' last batch with records ends in a tile of one record
    for name in U.A_NAMES:
        last = [b for b in table("A", name).batches() if b.n][-1]
        assert last.n % 1024 == 1, name
    # B: six groups of two full halves, then groups of 512 tiles and an empty batch
    for order in U.B_ORDERS:
        lay = [g.tile0 for _, g in U.expected_groups(table("B", order))]
        assert lay[:U.SETS] == [[0, 256, 512]] * U.SETS, order
        assert lay.count([0, 512, 512]) == 2 and lay[U.SETS + (order == "sync")] == [0, 512, 512], order
    assert [g.tile0 for _, g in U.expected_groups(table("B", "sync"))][U.SETS] == [0, 512]
    assert [g.tile0 for _, g in U.expected_groups(table("B", "read"))][-2:] == [[0, 1, 2]] * 2
    # C: no group of more than 256 tiles (the wide cell alone sends them to the general scan)
    for name in U.C_NAMES:
        assert max(g.T for _, g in U.expected_groups(table("C", name))) <= U.CHUNK, name
    lay = [g.tile0 for _, g in U.expected_groups(table("C", "wide-256-trailing-empty"))]
    assert lay == [[0, 128, 256]] * U.SETS + [[0, 256, 256]]
    # D: the third batch opens a group
    assert [g.tile0 for _, g in U.expected_groups(table("D"))] == [[0, 200, 400], [0, 200]]
    # F: one batch of 300 tiles a round
    assert U.tiles_of(U.f_batches(4)[0][0].n) == 300 > U.CHUNK


# ---- cells ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", ALL, ids=IDS)
def test_cells_at_the_switch_and_nowhere_else(kind, name):
    """Table C's named cells hold exactly 2^21 and 2^21 - 1 units; no other cell of any table is wide."""
    t = table(kind, name)
    named = {(o, j, tile, p): v for o, j, tile, p, v in t.notes.get("cells", [])}
    P = t.cfg["num_partitions"]
    seen = {}
    for o, op in enumerate(t.ops):
        if op[0] != "group":
            continue
        for j, b in enumerate(op[1]):
            if not b.n:
                continue
            cnt, b16 = U.cells(b, P)
            assert cnt.sum() == (b.pidx < P).sum()
            for tile, p in np.argwhere(b16 >= U.CELL_B16).tolist():
                seen[(o, j, tile, p)] = int(b16[tile][p])
                assert cnt[tile][p] == 1024
    assert seen == named, f"{t.name}: cells at or past 2^21 - 1 units"
    if kind == "C":
        assert any(v == 1 << 21 for v in seen.values())
    if name == "at-switch":
        assert sorted(seen.values()) == [(1 << 21) - 1, 1 << 21]


# ---- oracle -----------------------------------------------------------------------------------

def expected_stats(t: U.Table, o: int, j: int, b: Batch) -> dict:
    """By the table's own notes: every record of a known partition is appended, but those of a
    ShortBatch (all invalid) and of the (batch, partition) the table names as over S - I."""
    n, P = b.n, t.cfg["num_partitions"]
    want = dict(records=n, appended=0, rejected_not_leader=0, rejected_no_partition=0, rejected_no_space=0,
                rejected_invalid=0)
    if isinstance(b, U.ShortBatch):
        want["rejected_invalid"] = n
        return want
    want["rejected_no_partition"] = int((b.pidx >= P).sum())
    ns = t.notes.get("no_space")
    if ns and o == len(t.ops) - 1 and j == ns[0]:
        assert int((b.pidx == ns[1]).sum()) == ns[2]
        want["rejected_no_space"] = ns[2]
    want["appended"] = n - want["rejected_no_partition"] - want["rejected_no_space"]
    return want


def through_oracle(O, t: U.Table):
    """The table through the oracle and the model, batch by batch. Returns (model, per batch in
    submission order: {"pre": every partition's oracle state before it, "stats"}, final states)."""
    cfg = EngineConfig(**t.cfg)
    P = cfg.num_partitions
    model = U.FastPartitionModel(P, 1, cfg.segment_bytes)
    trace = []
    with O.OracleEngine(cfg) as ora:
        for o, op in enumerate(t.ops):
            if op[0] == "set_segments":
                ora.set_segments(op[1], op[2])
                model.set_segments(op[1], op[2])
                continue
            for j, b in enumerate(op[1]):
                pre = [ora.state(p) for p in range(P)]
                want = expected_stats(t, o, j, b)
                if isinstance(b, U.ShortBatch):
                    with pytest.raises(EngineError) as ex:
                        ora.append(b.pidx, b.lens, b.payload[:-1])
                    assert ex.value.status == A.RMQ_EINVAL
                    mo, ms = model.append(b.pidx, b.lens, invalid=True)
                else:
                    oo, so = ora.append(b.pidx, b.lens, b.payload)
                    mo, ms = model.append(b.pidx, b.lens)
                    assert so == want, f"{t.name} op {o} batch {j}: oracle stats {so}, the table expects {want}"
                    assert np.array_equal(mo, oo), f"{t.name} op {o} batch {j}: out offsets"
                assert ms == want, f"{t.name} op {o} batch {j}: model stats {ms}, the table expects {want}"
                trace.append({"pre": pre, "stats": ms})
            R.assert_model_agrees(model, ora, range(P), "oracle")
        final = [ora.state(p) for p in range(P)]
    return model, trace, final


@pytest.mark.parametrize("kind,name", ALL, ids=IDS)
def test_tables_through_oracle_and_model(oracle_mod, kind, name):
    t = table(kind, name)
    model, trace, final = through_oracle(oracle_mod, t)
    assert sum(e["stats"]["appended"] for e in trace) > 0
    if "invalid" in t.notes:
        assert sum(1 for e in trace if e["stats"]["rejected_invalid"]) == len(t.notes["invalid"])
    if "no_space" in t.notes:
        j, p, n = t.notes["no_space"]
        assert sum(e["stats"]["rejected_no_space"] for e in trace) == n
        # the partition took the batches around the one it refused
        grp = t.ops[-1][1]
        others = sum(int((b.pidx == p).sum()) for k, b in enumerate(grp) if k != j)
        before = trace[len(trace) - len(grp)]["pre"][p]["log_end_offset"]
        assert others and final[p]["log_end_offset"] - before == others
    if kind in ("B", "D") or name == "wide-256-trailing-empty":  # retention is at work
        assert final[0]["log_start_offset"] > 0, final[0]
    if name == "at-switch":
        assert [final[2]["log_end_offset"], final[2]["log_end_pos"]] == [2048, 2 * 33554432 - 16]
        assert trace[0]["stats"]["appended"] == 1024 and trace[1]["pre"][2]["log_end_pos"] == 33554432


# ---- sensitivity ------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", [("B", "wait"), ("C", "wide-256-trailing-empty")], ids=["B", "C-wide-256"])
def test_a_stale_aggregate_would_move_the_log_start(oracle_mod, kind, name):
    """For every group [X, empty] whose tiles end on a chunk boundary: FORMAT.md §4 replayed from the
    group's true per-batch aggregates gives the oracle's log start; with the empty batch's aggregate
    replaced by the second batch's of the group six earlier (the one that used the same scratch set),
    it gives another one."""
    t = table(kind, name)
    cfg = EngineConfig(**t.cfg)
    P, p = cfg.num_partitions, t.notes["part"]
    model, trace, final = through_oracle(oracle_mod, t)
    groups = U.expected_groups(t)
    batches = t.batches()
    seg = model.parts[p].seg
    room = [model.parts[q].seg - U.I for q in range(P)]
    aggs = [U.aggregates(batches[g.first:g.first + g.nb], P, room) for _, g in groups]

    def entry(m):
        try:
            return model.parts[p].E[m]
        except KeyError:
            return ("no entry", m)

    checked = 0
    for gi, (_, g) in enumerate(groups):
        if "trailing_empty_on_chunk" not in U.chunk_relations(g):
            continue
        assert gi >= U.SETS and groups[gi - U.SETS][1].nb == g.nb == 2
        pre = trace[g.first]["pre"][p]
        after = trace[g.first + g.nb]["pre"][p] if g.first + g.nb < len(trace) else final[p]
        start = (pre["log_start_offset"], pre["log_start_pos"])
        true = [a[p] for a in aggs[gi]]
        stale = [true[0], aggs[gi - U.SETS][1][p]]
        assert true[1] == true[0] and stale[1] != true[1]
        got = U.retention_replay(start, pre["log_end_pos"], seg, U.I, true, entry)
        assert got == (after["log_start_offset"], after["log_start_pos"]) and got != start
        bad = U.retention_replay(start, pre["log_end_pos"], seg, U.I, stale, entry)
        assert bad != got, f"group {gi}: a stale aggregate {stale[1]} leaves the log start where it belongs"
        checked += 1
    assert checked == (2 if kind == "B" else 1)
