"""Scenario builders for the ring-move sweeps (rmq_set_segments, FORMAT.md §2) — test infrastructure.

Each builder is deterministic (fixed seeds) and returns a Scenario: the engine config, the op
list in stages (tests/parity.py op tuples), the facts the scenario relies on, and per-stage guards
that assert on ORACLE state that the scenario still reaches the paths it was built for (a retained
window across a chunk boundary, a block that can only be a reused one, ...). play() runs the
stages on the oracle alone (tests/test_oracle_ring_moves.py, no GPU) or on an engine/oracle pair
through parity.run_ops with every ring compared whole (tests/test_gpu_ring_moves.py); the guards
run in both, so a scenario that has silently become vacuous fails without a GPU.

Sizes are derived from the config: chunks of MIGRATE_CHUNK new-ring bytes per workgroup of a move,
index rings of icap = (2 G + 2) S / I entries (parity.index_capacity).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from parity import compare_index_slots, compare_state, index_capacity, run_ops
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import EngineConfig, EngineError
from ripplemq_amd.workload import Batch

MIGRATE_CHUNK = 256 << 10  # kMigrateChunk (ripplemq_amd/csrc/kernels.hpp): new-ring bytes per workgroup
KiB = 1 << 10


def rec_bytes(ln: int) -> int:
    """FORMAT.md §1: 16-byte header + payload padded to 16."""
    return 16 + ((int(ln) + 15) & ~15)


def chunks_of(seg: int) -> int:
    return max(1, seg // MIGRATE_CHUNK)


def mixed_batch(g, want: dict, size) -> tuple[Batch, dict]:
    """One batch: for each partition p records of size[0]..size[1] bytes until their record bytes
    reach want[p] (it overshoots by less than one record), interleaved. Returns the batch and the
    record bytes each partition got."""
    lo, hi = size
    pidx, lens, got = [], [], {}
    for p, goal in want.items():
        n = 0
        while n < goal:
            ln = int(g.integers(lo, hi + 1))
            pidx.append(p)
            lens.append(ln)
            n += rec_bytes(ln)
        got[p] = n
    order = g.permutation(len(pidx))
    pidx = np.asarray(pidx, np.uint32)[order]
    lens = np.asarray(lens, np.uint32)[order]
    return Batch(pidx, lens, g.integers(0, 256, int(lens.sum()), dtype=np.uint8)), got


def fill_batches(g, targets: dict, per_batch: int, size, used: dict | None = None) -> tuple[list, dict]:
    """Batches of about per_batch record bytes per partition that take partition p's log end from
    used[p] (0) to just past targets[p]. Returns the batches and the log end positions reached."""
    used = dict(used or {})
    for p in targets:
        used.setdefault(p, 0)
    out = []
    while any(used[p] < t for p, t in targets.items()):
        b, got = mixed_batch(g, {p: min(per_batch, t - used[p]) for p, t in targets.items() if used[p] < t}, size)
        for p, n in got.items():
            used[p] += n
        out.append(b)
    return out, used


def fixed_batch(g, counts: dict, size=(33, 48)) -> Batch:
    """counts[p] records of size[0]..size[1] bytes for each partition (33..48 B: 64 bytes a record)."""
    pidx = np.concatenate([np.full(n, p, np.uint32) for p, n in counts.items()] + [np.zeros(0, np.uint32)])
    order = g.permutation(len(pidx))
    pidx = pidx[order]
    lens = g.integers(size[0], size[1] + 1, len(pidx)).astype(np.uint32)
    return Batch(pidx, lens, g.integers(0, 256, int(lens.sum()), dtype=np.uint8))


def appends(batches):
    return [("append", b) for b in batches]


def move(pidx, sizes):
    return ("set_segments", np.asarray(pidx, np.uint32), np.asarray(sizes, np.uint64))


@dataclass
class Scenario:
    cfg: EngineConfig
    stages: list                                  # [(name, [op, ...])]
    facts: dict = field(default_factory=dict)
    guards: dict = field(default_factory=dict)    # stage name -> fn(scenario, snaps, oracle)
    moved: dict = field(default_factory=dict)     # stage name -> partitions that stage's call moves
    quiet: tuple = ()                             # stages compared once at their end, not per op

    def records(self) -> int:
        return sum(len(op[1].pidx) for _, ops in self.stages for op in ops if op[0] == "append")


def apply_ops(ora, ops) -> None:
    """parity.run_ops' op list on the oracle alone."""
    for op in ops:
        kind = op[0]
        if kind == "append":
            b = op[1]
            ora.append(b.pidx, b.lens, b.payload)
        elif kind == "consumer_commit":
            ora.commit_consumer_offset(*op[1:4])
        elif kind == "fetch":
            ora.fetch(op[1], op[2], op[3], op[4] if len(op) > 4 else None, commit=bool(op[5]) if len(op) > 5 else False)
        elif kind == "set_segments":
            ora.set_segments(op[1], op[2])
        else:
            raise ValueError(kind)


def play(scn: Scenario, ora, dev=None, after=None) -> dict:
    """Run the stages in order; after each one take the oracle's partition states (snaps[name]), run
    the stage's guard and, with an engine, compare every index slot of the partitions the stage
    moved and call after[name](snaps). Returns the snaps."""
    P = scn.cfg.num_partitions
    snaps = {}
    for name, ops in scn.stages:
        if dev is None:
            apply_ops(ora, ops)
        else:
            run_ops(dev, ora, scn.cfg, ops, check=name not in scn.quiet, full_rings=True)
            if name in scn.quiet:
                compare_state(dev, ora, scn.cfg, full_rings=True)
        snaps[name] = [ora.state(p) for p in range(P)]
        if name in scn.guards:
            scn.guards[name](scn, snaps, ora)
        if dev is not None:
            for p in scn.moved.get(name, ()):
                compare_index_slots(dev, ora, scn.cfg, int(p))
            if after and name in after:
                after[name](snaps)
    return snaps


def window(st) -> tuple[int, int]:
    return st["log_start_pos"], st["log_end_pos"]


def retained_chunks(st) -> set:
    """Chunks (workgroups of a move) of the ring that hold a retained byte."""
    lo, hi = window(st)
    S, out = st["segment_bytes"], set()
    while lo < hi:
        out.add((lo % S) // MIGRATE_CHUNK)
        lo = (lo // MIGRATE_CHUNK + 1) * MIGRATE_CHUNK
    return out


def crosses(st, step: int, inner_of: int | None = None) -> bool:
    """Does a multiple of `step` lie strictly inside the retained window (inner_of: one that is no
    multiple of inner_of)?"""
    lo, hi = window(st)
    b = (lo // step + 1) * step
    while b < hi:
        if inner_of is None or b % inner_of:
            return True
        b += step
    return False


def live_shares(cfg, st) -> set:
    """Index shares (workgroups of a move) that hold a live entry: share of m = (m mod icap) nch / icap."""
    I, icap, nch = cfg.index_interval, index_capacity(cfg, st["segment_bytes"]), chunks_of(st["segment_bytes"])
    m_lo, m_hi = -(-st["log_start_pos"] // I), st["log_end_pos"] // I
    return {(m % icap) * nch // icap for m in range(m_lo, m_hi + 1)}


def ring_spans(lo: int, hi: int, S: int) -> list:
    """Ring offset intervals of logical positions [lo, hi), hi - lo <= S."""
    if hi <= lo:
        return []
    a, n = lo % S, hi - lo
    return [(a, a + n)] if a + n <= S else [(a, S), (0, a + n - S)]


def all_appended(scn, snaps, ora) -> None:
    """No batch was rejected for space: every submitted record got an offset."""
    got = sum(ora.state(p)["log_end_offset"] for p in range(scn.cfg.num_partitions))
    assert got == scn.records(), (got, scn.records())


# ---------------------------------------------------------------------------------------------
# 1. Multi-chunk grow on data
# ---------------------------------------------------------------------------------------------

def multi_chunk_grow(new_seg: int) -> Scenario:
    """Three partitions filled through 64 KiB rings to just past 3, 4 and 5 chunks of logical position
    and a fourth with a short log, grown into rings of several chunks: retained windows in chunks
    c >= 1, across a chunk boundary and across the new ring's end, live index entries in shares
    c >= 1 and across a share boundary, chunks that only write zeros."""
    S, K = 64 * KiB, MIGRATE_CHUNK
    cfg = EngineConfig(num_partitions=6, replication_factor=2, segment_bytes=S, index_interval=1024,
                       max_consumers=2, max_batch_records=4096, pipeline_depth=1, pool_bytes=4 << 20)
    g = np.random.default_rng(101)
    levels = {0: 3 * K, 2: 4 * K, 4: 5 * K}
    short = 1
    targets = dict(levels)
    targets.update({short: 20 * KiB, 3: 30 * KiB, 5: 8 * KiB})
    fill, used = fill_batches(g, targets, 48 * KiB, (1, 700))
    grown = [4, 0, 2, short]
    sizes = [new_seg, new_seg, new_seg, 2 * K]
    more, _ = fill_batches(g, {p: used[p] + 96 * KiB for p in range(6)}, 48 * KiB, (1, 700), used)
    assert len(more) == 2
    scn = Scenario(cfg, [("fill", appends(fill)), ("move", [move(grown, sizes)]), ("more", appends(more))],
                   facts=dict(levels=levels, grown=grown, sizes=sizes, used=used),
                   moved={"move": grown}, quiet=("fill",))

    def guard(scn, snaps, ora):
        st = snaps["move"]
        for p, lv in levels.items():
            assert lv < st[p]["log_end_pos"] <= lv + 1024, (p, st[p])   # just past its level
            assert st[p]["segment_bytes"] == new_seg and chunks_of(new_seg) >= 2
            assert st[p]["log_start_offset"] > 0                        # it wrapped its first ring
        assert st[short]["segment_bytes"] == 2 * K
        assert snaps["fill"] == [dict(s, segment_bytes=S) for s in st], "a grow evicts nothing"
        mv = [st[p] for p in grown]
        assert any(crosses(s, K, s["segment_bytes"]) for s in mv), "no window crosses an interior chunk boundary"
        assert any(crosses(s, s["segment_bytes"]) for s in mv), "no window wraps the new ring's end"
        shares = [live_shares(cfg, s) for s in mv]
        assert any(len(x) >= 2 for x in shares), "no live entries on both sides of a share boundary"
        assert any(len(x) == 1 and min(x) >= 1 for x in shares), "no live entries wholly inside a share c >= 1"
        assert any(set(range(1, chunks_of(s["segment_bytes"]))) - retained_chunks(s) for s in mv), \
            "every chunk c >= 1 holds a retained byte"
        assert sum(max(retained_chunks(s)) >= 1 for s in mv) >= 3, "too few chunks c >= 1 copy a byte"

    scn.guards = {"move": guard, "more": all_appended}
    return scn


# ---------------------------------------------------------------------------------------------
# 2. Dirty block reuse
# ---------------------------------------------------------------------------------------------

def dirty_block_reuse() -> Scenario:
    """X grows into the only block of `big` bytes the pool can give, more than `big` bytes pass
    through it, X shrinks (the block is freed dirty), and Y, a short log at other ring offsets, grows
    to `big`: its ring and index ring must be zero outside what it retains."""
    S, big, P = 64 * KiB, 1 << 20, 6
    cfg = EngineConfig(num_partitions=P, replication_factor=2, segment_bytes=S, index_interval=1024,
                       max_consumers=2, max_batch_records=4096, pipeline_depth=1, pool_bytes=2 << 20)
    g = np.random.default_rng(102)
    X, Y = 1, 4
    seed, used = fill_batches(g, {X: 30 * KiB, Y: 20 * KiB, 0: 10 * KiB}, 48 * KiB, (1, 700))
    dirty, used = fill_batches(g, {X: used[X] + big + 100 * KiB}, 200 * KiB, (1, 700), used)
    more, _ = fill_batches(g, {X: used[X] + 60 * KiB, Y: used[Y] + 60 * KiB}, 30 * KiB, (1, 700), used)
    stages = [("seed", appends(seed)), ("grow_x", [move([X], [big])]), ("dirty", appends(dirty)),
              ("shrink_x", [move([X], [S])]), ("grow_y", [move([Y], [big])]), ("more", appends(more))]
    # blocks of `big` bytes that no creation-time ring lies in (FORMAT.md §2: blocks are aligned to
    # their size, partition p starts in block p * segment_bytes, no coalescing)
    free_big = cfg.pool_bytes // big - -(-P * S // big)
    scn = Scenario(cfg, stages, facts=dict(X=X, Y=Y, big=big, free_big_blocks=free_big),
                   moved={"grow_x": [X], "shrink_x": [X], "grow_y": [Y]}, quiet=("dirty",))

    def guard_y(scn, snaps, ora):
        assert scn.facts["free_big_blocks"] == 1, "Y's grow need not reuse X's block"
        x0, x1, x2 = snaps["grow_x"][X], snaps["dirty"][X], snaps["shrink_x"][X]
        assert x1["log_end_pos"] - x0["log_end_pos"] > big, "X did not dirty its whole block"
        assert x1["log_end_pos"] - x1["log_start_pos"] > S and x2["log_start_offset"] > x1["log_start_offset"]
        y = snaps["grow_y"][Y]
        assert (x2["segment_bytes"], y["segment_bytes"]) == (S, big)
        ys = ring_spans(*window(y), big)
        xs = ring_spans(*window(x2), big)  # where the log X kept lay in the block it left
        assert ys and all(b <= c or d <= a for a, b in ys for c, d in xs), "Y lands on X's last window"
        assert y["log_end_pos"] - y["log_start_pos"] < big // 8

    scn.guards = {"grow_y": guard_y, "more": all_appended}
    return scn


# ---------------------------------------------------------------------------------------------
# 3. Mixed items in one call
# ---------------------------------------------------------------------------------------------

def mixed_items() -> Scenario:
    """One call of seven unsorted items: new rings of 1, 4, 2, 1, 2 and 1 chunks, grows and shrinks
    together, all on data, and one item that has the requested size already (skipped: the chunk
    prefix of the items after it must still line up)."""
    S, K = 64 * KiB, MIGRATE_CHUNK
    cfg = EngineConfig(num_partitions=8, replication_factor=3, segment_bytes=S, index_interval=1024,
                       max_consumers=2, max_batch_records=4096, pipeline_depth=1, pool_bytes=4 << 20)
    g = np.random.default_rng(103)
    targets = {5: 100 * KiB, 2: 7 * K // 2, 0: 60 * KiB, 7: 7 * K // 4, 3: 150 * KiB, 6: 13 * K // 4, 1: 90 * KiB,
               4: 30 * KiB}
    fill, used = fill_batches(g, targets, 48 * KiB, (1, 700))
    pidx = [5, 2, 0, 7, 3, 6, 1]
    sizes = [16 * KiB, 4 * K, S, 2 * K, 4 * KiB, 2 * K, 128 * KiB]
    # per-partition bytes of a batch stay below the smallest ring less an interval (no rejection)
    step = {p: 40 * KiB for p in range(8)}
    step.update({5: 10 * KiB, 3: 2 * KiB})
    m1, used = fill_batches(g, {p: used[p] + step[p] for p in range(8)}, 48 * KiB, (1, 700), used)
    m2, used = fill_batches(g, {p: used[p] + step[p] for p in range(8)}, 48 * KiB, (1, 700), used)
    assert len(m1) == len(m2) == 1
    real = [(p, s) for p, s in zip(pidx, sizes) if s != S]
    scn = Scenario(cfg, [("fill", appends(fill)), ("move", [move(pidx, sizes)]), ("more", appends(m1 + m2))],
                   facts=dict(pidx=pidx, sizes=sizes, chunk_counts=[chunks_of(s) for _, s in real]),
                   moved={"move": [p for p, _ in real]}, quiet=("fill",))

    def guard(scn, snaps, ora):
        before, st = snaps["fill"], snaps["move"]
        assert scn.facts["chunk_counts"][:5] == [1, 4, 2, 1, 2] and len(pidx) >= 6
        assert pidx != sorted(pidx) and sum(s == S for s in sizes) == 1
        assert sizes[pidx.index(0)] == S and 0 < pidx.index(0) < len(pidx) - 1  # items on both sides of the skip
        for p, s in zip(pidx, sizes):
            assert st[p]["segment_bytes"] == s and st[p]["log_end_offset"] > 0, (p, st[p])
        grows = [p for p, s in real if s > S]
        shrinks = [p for p, s in real if s < S]
        assert len(grows) >= 2 and len(shrinks) >= 2
        for p in shrinks:  # a shrink on data applies retention
            assert st[p]["log_start_offset"] > before[p]["log_start_offset"], p
            assert 0 < st[p]["log_end_pos"] - st[p]["log_start_pos"] <= st[p]["segment_bytes"]
        for p, s in real:  # an item taken for another, or a chunk for another, copies the wrong bytes
            if chunks_of(s) > 1:
                assert min(retained_chunks(st[p])) >= 1, (p, retained_chunks(st[p]))

    scn.guards = {"move": guard, "more": all_appended}
    return scn


# ---------------------------------------------------------------------------------------------
# 4. Shrink edges
# ---------------------------------------------------------------------------------------------

EDGE_KINDS = ("exact", "plus_one_record", "evict_on_interval", "end_on_interval")


def shrink_edges(new_seg: int) -> Scenario:
    """Eight logs of 64-byte records (33..48 B payloads) in 16 KiB rings, I = 256, shrunk to new_seg
    in one call. Partition 2 k + w has edge kind k; w = 1 first passes three rings' worth of records,
    shrinks to 4 I and grows back, so that its log start B is far from 0 (w = 0: B = 0). With
    L = log_end_pos - B before the shrink:
      exact              L = S': nothing is evicted, the new ring is full, the start stays;
      plus_one_record    L = S' + 64: the start moves one interval, to B + I;
      evict_on_interval  L = S' + I: log_end_pos - S' is an interval multiple and a record starts there;
      end_on_interval    L = S' + 3 I, log_end_pos an interval multiple: the last live entry names
                         the record the next append writes.
    (S' is a multiple of I, so log_end_pos - S' is an interval multiple exactly when log_end_pos is:
    the last two kinds differ in how much is evicted.)"""
    S, I, R = 16 * KiB, 256, 64
    cfg = EngineConfig(num_partitions=8, replication_factor=3, segment_bytes=S, index_interval=I,
                       max_consumers=2, max_batch_records=4096, pipeline_depth=1, pool_bytes=512 * KiB)
    g = np.random.default_rng(104 + new_seg // KiB)
    parts = {2 * k + w: (EDGE_KINDS[k], w) for k in range(4) for w in (0, 1)}
    level = {"exact": new_seg, "plus_one_record": new_seg + R, "evict_on_interval": new_seg + I,
             "end_on_interval": new_seg + 3 * I}
    wrapped = [p for p, (_, w) in parts.items() if w]
    base = 3 * S  # log end of the wrapped logs before their first shrink, an interval multiple
    wrap = [fixed_batch(g, {p: S // R * 3 // 4 for p in wrapped}) for _ in range(4)]
    B = {p: (base - 4 * I if w else 0) for p, (_, w) in parts.items()}
    have = {p: (4 * I if w else 0) for p, (_, w) in parts.items()}
    lvl = fixed_batch(g, {p: (level[k] - have[p]) // R for p, (k, _) in parts.items()})
    more = [fixed_batch(g, {p: 8 for p in parts}) for _ in range(2)]
    allp = sorted(parts)
    stages = [("wrap", appends(wrap)), ("pre_shrink", [move(wrapped, [4 * I] * 4)]),
              ("pre_grow", [move(wrapped, [S] * 4)]), ("level", [("append", lvl)]),
              ("move", [move(allp, [new_seg] * 8)]), ("more", appends(more))]
    scn = Scenario(cfg, stages, facts=dict(parts=parts, level=level, B=B, new_seg=new_seg),
                   moved={"pre_shrink": wrapped, "pre_grow": wrapped, "move": allp})

    def guard_level(scn, snaps, ora):
        for p, (k, w) in parts.items():
            st = snaps["level"][p]
            assert (st["log_start_pos"], st["log_end_pos"]) == (B[p], B[p] + level[k]), (p, k, w, st)
            assert st["segment_bytes"] == S and (st["log_start_offset"] > 0) == bool(w)

    def guard_move(scn, snaps, ora):
        for p, (k, w) in parts.items():
            b, st = snaps["level"][p], snaps["move"][p]
            used, keep = b["log_end_pos"], st["log_end_pos"] - st["log_start_pos"]
            assert st["segment_bytes"] == new_seg and st["log_end_pos"] == used
            assert ora.record_pos(p, st["log_start_offset"]) == st["log_start_pos"]
            if k == "exact":
                assert keep == new_seg, (p, st)
                assert (st["log_start_offset"], st["log_start_pos"]) == (b["log_start_offset"], b["log_start_pos"])
            elif k == "plus_one_record":
                assert st["log_start_pos"] == B[p] + I and keep == new_seg - (I - R), (p, st)
            else:
                assert (used - new_seg) % I == 0 and st["log_start_pos"] == used - new_seg and keep == new_seg, (p, st)
                assert st["log_start_offset"] > b["log_start_offset"]
            if used % I == 0:  # the last live entry names a record that does not exist yet
                assert ora.read_index(p, used // I, 1).tolist() == [[st["log_end_offset"], used]], p
        assert sum(snaps["level"][p]["log_end_pos"] % I == 0 for p in parts) >= 6

    def guard_more(scn, snaps, ora):
        all_appended(scn, snaps, ora)
        for p in parts:  # the record the last live entry named exists now
            b, st = snaps["move"][p], snaps["more"][p]
            assert st["log_end_offset"] == b["log_end_offset"] + 16
            assert ora.record_pos(p, b["log_end_offset"]) == b["log_end_pos"]

    scn.guards = {"level": guard_level, "move": guard_move, "more": guard_more}
    return scn


def shrink_misc() -> Scenario:
    """A last record longer than the new ring (the retained log is empty, the ring all zeros), a
    partition that never took a record grown and shrunk, and a log that wrapped its ring many times
    shrunk to 4 I."""
    S, I = 64 * KiB, 1024
    cfg = EngineConfig(num_partitions=4, replication_factor=2, segment_bytes=S, index_interval=I,
                       max_consumers=3, max_batch_records=4096, pipeline_depth=1, pool_bytes=1 << 20)
    g = np.random.default_rng(105)
    LONG, EMPTY, WRAPPED, REST = 0, 1, 2, 3
    fill, used = fill_batches(g, {LONG: 20 * KiB, WRAPPED: 10 * S + 5 * KiB, REST: 10 * KiB}, 48 * KiB, (1, 300))
    long_rec = Batch(np.array([LONG], np.uint32), np.array([16000], np.uint32), g.integers(0, 256, 16000, dtype=np.uint8))
    nrec = sum(int((b.pidx == LONG).sum()) for b in fill) + 1
    pp = np.full(3, LONG, np.uint32)
    cc = np.arange(3, dtype=np.uint32)
    reads = [("consumer_commit", pp[1:], cc[1:], np.array([nrec - 1, nrec], np.uint64)),
             ("fetch", pp, cc, np.full(3, 10, np.uint32))]  # consumer 0 at offset 0: evicted long ago
    more = [mixed_batch(g, {p: 2 * KiB for p in range(4)}, (1, 300))[0] for _ in range(2)]
    stages = [("fill", appends(fill) + [("append", long_rec)]),
              ("move", [move([WRAPPED, LONG, EMPTY], [4 * I, 4 * KiB, 256 * KiB])]), ("reads", reads),
              ("shrink_empty", [move([EMPTY], [4 * I])]), ("more", appends(more)), ("reads2", reads[1:])]
    scn = Scenario(cfg, stages, facts=dict(long=LONG, empty=EMPTY, wrapped=WRAPPED, long_records=nrec),
                   moved={"move": [WRAPPED, LONG, EMPTY], "shrink_empty": [EMPTY]}, quiet=("fill",))

    def guard(scn, snaps, ora):
        b, st = snaps["fill"], snaps["move"]
        assert rec_bytes(16000) > 4 * KiB and b[LONG]["log_end_offset"] == nrec
        s = st[LONG]
        assert s["log_start_offset"] == s["log_end_offset"] == nrec and s["log_start_pos"] == s["log_end_pos"]
        for r in range(cfg.replication_factor):
            assert not ora.read_segment(r, LONG).any(), "the ring of an empty retained log is all zeros"
        assert st[EMPTY]["log_end_pos"] == 0 and st[EMPTY]["segment_bytes"] == 256 * KiB
        w = st[WRAPPED]
        assert b[WRAPPED]["log_end_pos"] > 10 * S and w["segment_bytes"] == 4 * I
        assert 0 < w["log_end_pos"] - w["log_start_pos"] <= 4 * I and w["log_start_offset"] > b[WRAPPED]["log_start_offset"]

    def guard_end(scn, snaps, ora):
        all_appended(scn, snaps, ora)
        assert snaps["more"][EMPTY]["segment_bytes"] == 4 * I and snaps["more"][EMPTY]["log_end_offset"] > 0

    scn.guards = {"move": guard, "more": guard_end}
    return scn


# ---------------------------------------------------------------------------------------------
# 5. Fetch across moves
# ---------------------------------------------------------------------------------------------

def fetch_across_moves() -> Scenario:
    """One consumer reads one partition 10 records at a time with RMQ_FETCH_COMMIT; between reads the
    ring grows, shrinks keeping the consumer's next record, and shrinks evicting it (the next read
    answers RMQ_EOFFSET with the first retained offset, its commit takes it, and the reads go on to
    the log end)."""
    S, I = 64 * KiB, 1024
    cfg = EngineConfig(num_partitions=2, replication_factor=2, segment_bytes=S, index_interval=I,
                       max_consumers=1, max_batch_records=4096, pipeline_depth=1, pool_bytes=1 << 20)
    g = np.random.default_rng(106)
    fill = [fixed_batch(g, {0: 110, 1: 20}, (1, 180)) for _ in range(3)]
    total = 330
    one = np.zeros(1, np.uint32)
    F = ("fetch", one, one, np.full(1, 10, np.uint32), None, True)
    stages = [("fill", appends(fill)), ("read1", [F] * 3), ("grow", [move([0], [4 * S])]), ("read2", [F] * 8),
              ("shrink_keep", [move([0], [S // 2])]), ("read3", [F] * 2), ("shrink_evict", [move([0], [4 * I])]),
              ("resume", [F]), ("read4", [F] * 8)]
    scn = Scenario(cfg, stages, facts=dict(total=total),
                   moved={"grow": [0], "shrink_keep": [0], "shrink_evict": [0]})

    def cons(ora):
        return int(ora.consumer_offsets(0)[0])

    def g_keep(scn, snaps, ora):
        st = snaps["shrink_keep"][0]
        assert cons(ora) == 110 and 0 < st["log_start_offset"] <= cons(ora), (st, cons(ora))

    def g_evict(scn, snaps, ora):
        st = snaps["shrink_evict"][0]
        assert cons(ora) == 130 < st["log_start_offset"] < total - 10, (st, cons(ora))

    def g_resume(scn, snaps, ora):  # RMQ_EOFFSET names the first retained offset and the commit takes it
        assert cons(ora) == snaps["shrink_evict"][0]["log_start_offset"]

    def g_end(scn, snaps, ora):
        assert cons(ora) == total == snaps["read4"][0]["log_end_offset"]

    scn.guards = {"shrink_keep": g_keep, "shrink_evict": g_evict, "resume": g_resume, "read4": g_end}
    return scn


# ---------------------------------------------------------------------------------------------
# 6. Moves with the pipeline in flight
# ---------------------------------------------------------------------------------------------

def pipelined_moves(depth: int, late: bool) -> Scenario:
    """depth + 1 (depth 2) or depth + 2 (depth 3) batches, a call that grows partition 0 and shrinks
    partition 1, three more batches. late: the batches of the last launch group before the call add
    more than a ring less an interval to partition 1 (each batch alone fits), so that group's
    retention of partition 1 cannot finish inside its own launch."""
    S, I = 64 * KiB, 1024
    cfg = EngineConfig(num_partitions=4, replication_factor=2, segment_bytes=S, index_interval=I,
                       max_consumers=2, max_batch_records=4096, pipeline_depth=depth, pool_bytes=1 << 20)
    g = np.random.default_rng(107 + 10 * depth + late)
    n = depth + (1 if depth == 2 else 2)
    tail = n % depth  # batches of the last group
    assert tail and (not late or tail >= 2)
    before, per1 = [], []
    for k in range(n):
        want = {p: 25 * KiB for p in range(4)}
        if late and k >= n - tail:
            want[1] = 40 * KiB
        b, got = mixed_batch(g, want, (1, 300))
        before.append(b)
        per1.append(got[1])
    after = [mixed_batch(g, {0: 20 * KiB, 1: 10 * KiB, 2: 20 * KiB, 3: 20 * KiB}, (1, 300))[0] for _ in range(3)]
    stages = [("before", appends(before)), ("move", [move([1, 0], [16 * KiB, 8 * S])]), ("after", appends(after))]
    scn = Scenario(cfg, stages, facts=dict(depth=depth, late=late, last_group_bytes=sum(per1[n - tail:])),
                   moved={"move": [1, 0]})

    def guard(scn, snaps, ora):
        assert n % depth and max(per1) <= S - I
        assert (scn.facts["last_group_bytes"] > S - I) == late
        b, st = snaps["before"][1], snaps["move"][1]
        assert st["segment_bytes"] == 16 * KiB and st["log_start_offset"] > b["log_start_offset"]
        assert snaps["move"][0]["segment_bytes"] == 8 * S and snaps["move"][0]["log_start_offset"] > 0

    scn.guards = {"move": guard, "after": all_appended}
    return scn


# ---------------------------------------------------------------------------------------------
# 7. Refused calls
# ---------------------------------------------------------------------------------------------

def refused_calls() -> Scenario:
    """A filled engine whose pool has one free block of 4 S bytes. facts["calls"]: (name, pidx, sizes,
    status, does the oracle judge it); each refused call names a valid grow first, so a call that
    allocated before it refused would leak the block the final grow needs."""
    S, I = 64 * KiB, 1024
    cfg = EngineConfig(num_partitions=4, replication_factor=2, segment_bytes=S, index_interval=I,
                       max_consumers=2, max_batch_records=4096, pipeline_depth=1, pool_bytes=8 * S)
    g = np.random.default_rng(108)
    fill, _ = fill_batches(g, {p: (30 + 25 * p) * KiB for p in range(4)}, 48 * KiB, (1, 300))
    big = 4 * S
    calls = [("duplicate", [0, 1, 0], [big, 16 * KiB, big], A.RMQ_EINVAL, True),
             ("not_pow2", [0, 1], [big, 48 * KiB], A.RMQ_EINVAL, True),
             ("below_4_intervals", [0, 1], [big, 2 * I], A.RMQ_EINVAL, True),
             ("above_pool", [0, 1], [big, 2 * cfg.pool_bytes], A.RMQ_EINVAL, False),
             ("no_partition", [0, 4], [big, 16 * KiB], A.RMQ_ENOPART, True),
             ("empty", [], [], A.RMQ_OK, True)]
    more = [mixed_batch(g, {p: 20 * KiB for p in range(4)}, (1, 300))[0]]
    scn = Scenario(cfg, [("fill", appends(fill)), ("grow", [move([0], [big])]), ("more", appends(more))],
                   facts=dict(calls=calls, big=big), moved={"grow": [0]}, quiet=("fill",))

    def guard(scn, snaps, ora):
        assert cfg.pool_bytes // big - -(-4 * S // big) == 1, "a leaked block would go unnoticed"
        assert snaps["grow"][0]["segment_bytes"] == big
        assert all(s["log_end_offset"] > 0 for s in snaps["fill"])

    scn.guards = {"grow": guard, "more": all_appended}
    return scn


def call_status(eng, pidx, sizes) -> int:
    try:
        eng.set_segments(np.asarray(pidx, np.uint32), np.asarray(sizes, np.uint64))
    except EngineError as ex:
        return ex.status
    return A.RMQ_OK


# ---------------------------------------------------------------------------------------------
# 8. A follower whose ring differs from its leader's
# ---------------------------------------------------------------------------------------------

@dataclass
class FollowerScript:
    world: int
    rf: int
    ppr: int
    group: int
    rounds: int
    move_after: int   # rounds before the moves (every rank syncs there)
    views: list
    cfgs: list
    batches: list     # [rank][rounds * group]
    moves: list       # [rank] (pidx, sizes) or None


def follower_ring_script() -> FollowerScript:
    """tests/test_gpu_replication.scenario's shape (world 3, RF 3, 4 partitions led per rank, launch
    groups of 2, 64 KiB rings, I = 256) with ring moves on two of the ranks after round 3: rank 1
    grows the partitions it leads to 512 KiB and shrinks the ones it follows to 32 KiB, rank 0 moves
    one led and one followed partition, rank 2 none. A follower then ingests, indexes and retains
    through a ring of another size than its leader's."""
    from repl_sim import rank_batches, rank_cfg
    from ripplemq_amd.sharding import rank_view
    from ripplemq_amd.workload import StreamSpec
    world, rf, ppr, group, rounds = 3, 3, 4, 2, 6
    S = 64 * KiB
    base = EngineConfig(num_partitions=1, replication_factor=rf, segment_bytes=S, index_interval=256,
                        max_batch_records=4096, max_batch_bytes=1 << 20, pipeline_depth=group, pool_bytes=4 << 20)
    views = [rank_view(r, world, ppr, rf) for r in range(world)]
    cfgs = [rank_cfg(base, views[r], r) for r in range(world)]
    spec = StreamSpec(ppr, 400, "uniform", size=(1, 200), config_index=109)
    batches = [rank_batches(spec, r, rounds, group) for r in range(world)]
    n1 = len(views[1].gp)
    moves = [([0, ppr + 1], [4 * S, S // 2]),
             (list(range(n1)), [8 * S] * ppr + [S // 2] * (n1 - ppr)),
             None]
    return FollowerScript(world, rf, ppr, group, rounds, 3, views, cfgs, batches, moves)


def run_follower_oracles(oras, fs: FollowerScript) -> None:
    """The script on per-rank oracles (tests/repl_sim.py): a launch group's batches form one round;
    the sync before the moves and the last one exchange commit notices."""
    from repl_sim import exchange_round, notice_round, place
    for r in range(fs.world):
        place(oras[r], fs.views[r], fs.world)
    for k in range(fs.rounds):
        if k == fs.move_after:
            notice_round(oras)
            for r in range(fs.world):
                if fs.moves[r]:
                    oras[r].set_segments(*fs.moves[r])
        for r in range(fs.world):
            for b in fs.batches[r][k * fs.group:(k + 1) * fs.group]:
                oras[r].append(b.pidx, b.lens, b.payload)
        exchange_round(oras)
    notice_round(oras)


def follower_guards(oras, fs: FollowerScript) -> None:
    I = fs.cfgs[0].index_interval
    ring = {}  # global partition -> smallest ring on any rank
    for r in range(fs.world):
        for p, gp in enumerate(fs.views[r].gp):
            seg = oras[r].state(p)["segment_bytes"]
            ring[int(gp)] = min(ring.get(int(gp), seg), seg)
    assert min(ring.values()) == 32 * KiB
    for r in range(fs.world):  # no round carries more for a partition than its smallest ring less an interval
        for k in range(fs.rounds):
            per = np.zeros(fs.ppr, np.int64)
            for b in fs.batches[r][k * fs.group:(k + 1) * fs.group]:
                rs = 16 + ((b.lens.astype(np.int64) + 15) & ~15)
                per += np.bincount(b.pidx, weights=rs, minlength=fs.ppr).astype(np.int64)
            for p in range(fs.ppr):
                assert per[p] <= ring[r * fs.ppr + p] - I, (r, k, p, per[p])
    ahead = 0  # shrunk follower rings that applied retention their leader has not
    for r in range(fs.world):
        for p, gp in enumerate(fs.views[r].gp):
            lead, lp = int(gp) // fs.ppr, int(gp) % fs.ppr
            if lead == r:
                continue
            f, l = oras[r].state(p), oras[lead].state(lp)
            assert f["log_end_offset"] == l["log_end_offset"] > 0, (r, p)
            if f["segment_bytes"] < l["segment_bytes"] and f["log_start_offset"] > l["log_start_offset"]:
                ahead += 1
    assert ahead >= 1, "no shrunk follower ring retains less than its leader"
    for r in range(fs.world):
        c = oras[r].counters()
        assert int(c[1]) == 0 and int(c[2]) == 0, (r, c)
        for p in range(fs.views[r].led):
            s = oras[r].state(p)
            assert s["commit"] == s["log_end_offset"] > 0, (r, p, s)
