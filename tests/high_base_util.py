"""High coordinates: partitions rebased to offsets and logical positions past 2^31, 2^32, 2^53 and
2^58, and the CPU oracle translated to them. Shared by tests/test_high_base_model.py (CPU) and
tests/test_gpu_high_base.py.

rmq_restore with an empty run restarts a pristine partition as an empty log at any (first_offset,
first_pos) below 2^59 (FORMAT.md §11). The oracle has no restore and starts at (0, 0), but FORMAT.md
§§1-8 are translation-invariant: rebase partition p to (dO, dP) with dP a multiple of the index
interval I, run the same operations on the oracle from (0, 0), and

  * every offset the engine reports is the oracle's plus dO (RMQ_OFFSET_NONE and a remote slot's
    untouched match of 0 stay), every logical position the oracle's plus dP;
  * the retained window [log_start_pos, log_end_pos), read out of the ring at pos mod S, is the
    oracle's window byte for byte but for each record's 8-byte header offset, which is the oracle's
    plus dO (the CRC covers the payload only); retention decides alike because dP = 0 (mod I);
  * index entry E[m + dP / I] is the oracle's E[m] plus (dO, dP);
  * a fetch answers the oracle's rows with start_offset moved and the header offsets restamped;
    statuses, count, bytes, out_pos and bytes_used are unchanged.

Translated presents the translated oracle through the oracle's own interface, so parity.run_ops,
compare_state and pipelined take it in the oracle's seat. Every sum of the translation is taken
over Python integers. Bytes outside the retained window cannot be restamped (their records are
gone), so these tests compare windows (full_rings=False).
"""
from __future__ import annotations

import numpy as np

from ripplemq_amd import _abi as A
from ripplemq_amd.engine import RESTORE_ITEM_DTYPE, EngineConfig
from ripplemq_amd.tier import record_positions
from ripplemq_amd.workload import Batch, StreamSpec, make_batch

NONE = A.RMQ_OFFSET_NONE
OFFSET_FIELDS = ("log_start_offset", "log_end_offset", "commit", "high_watermark", "leader_commit", "term_start")
POS_FIELDS = ("log_start_pos", "log_end_pos")
_MOVED = (A.RMQ_OK, A.RMQ_EOFFSET, A.RMQ_ENOSPC)  # fetch rows whose start_offset is an offset of the log


def bases_for(I: int) -> dict:
    """{partition: (dO, dP)} of the issue, every dP a multiple of I; partition 0 stays at (0, 0) as
    the control, 6 and 7 repeat the two bases around 2^32 (two partitions per base in one engine)."""
    b = {0: (0, 0),
         1: (2 ** 32 - 37, 2 ** 32 - 3 * I),   # offsets and positions cross 2^32 inside the first batch
         2: (2 ** 32 + 5, 2 ** 32),
         3: (2 ** 31 - 11, 2 ** 31 - I),       # the signed boundary
         4: (2 ** 53 + 1, 2 ** 53 + 5 * I),    # past double's integers
         5: (2 ** 58 + 1, 2 ** 58 + 7 * I),    # the top of the ack word's range (FORMAT.md §9)
         6: (2 ** 32 - 37, 2 ** 32 - 3 * I),
         7: (2 ** 32 + 5, 2 ** 32)}
    assert all(dp % I == 0 for _, dp in b.values())
    return b


CROSSING = {1: 2 ** 32, 6: 2 ** 32, 3: 2 ** 31}  # partition: the boundary its base crosses


def cfg_high(**kw) -> EngineConfig:
    d = dict(num_partitions=8, replication_factor=3, segment_bytes=1 << 16, index_interval=256, max_consumers=4,
             max_batch_records=1024, max_batch_bytes=1 << 20, pipeline_depth=2)
    d.update(kw)
    return EngineConfig(**d)


def rebase(eng, bases, ora=None, lead_term=2):
    """One rmq_restore of empty runs puts every partition p of `bases` at bases[p] (a partition at
    (0, 0) is left as it was created); every consumer offset and the replica cursor of a rebased
    partition then start at its first offset, as the oracle's start at 0. rmq_become_leader follows
    on the engine and on the oracle `ora` alike, for every partition of `bases`, so that term_start
    translates."""
    every = sorted(bases)
    parts = [p for p in every if tuple(bases[p]) != (0, 0)]
    if parts:
        items = np.zeros(len(parts), RESTORE_ITEM_DTYPE)
        for k, p in enumerate(parts):
            dO, dP = bases[p]
            items[k] = (p, 0, dO, dP, 0, 0, 0, 0, dO)
        rows = eng.restore(items, np.zeros(0, np.uint8), np.zeros(1, np.uint64))
        assert [int(r["status"]) for r in rows] == [A.RMQ_OK] * len(parts), rows
        nc = eng.cfg.max_consumers
        pp = np.repeat(np.array(parts, np.uint32), nc)
        rc, st = eng.commit_consumer_offset(pp, np.tile(np.arange(nc, dtype=np.uint32), len(parts)),
                                            np.array([bases[int(p)][0] for p in pp], np.uint64))
        assert rc == 0 and not st.any(), (rc, st)
        eng.set_replica_cursor(np.array(parts, np.uint32), np.array([bases[p][0] for p in parts], np.uint64))
    if lead_term is not None:
        for e in (eng, ora):
            if e is not None:
                rebase_oracle(e, bases, lead_term)


def restamp_records(buf: np.ndarray, shift) -> None:
    """In place: the header offset h of every FORMAT.md §1 record that fills buf becomes shift(h). A
    plain walk over the length words."""
    pos, n = 0, buf.size
    while pos < n:
        h = int.from_bytes(buf[pos:pos + 8].tobytes(), "little")
        ln = int.from_bytes(buf[pos + 8:pos + 12].tobytes(), "little")
        buf[pos:pos + 8] = np.frombuffer(int(shift(h)).to_bytes(8, "little"), np.uint8)
        pos += 16 + ((ln + 15) & ~15)
    assert pos == n, (pos, n)


class Translated:
    """The oracle `ora`, run from (0, 0), seen at bases {p: (dO, dP)} (partitions not named stay at
    (0, 0)). rebase() is assumed on the engine it is compared with: every consumer offset of a
    rebased partition counts as committed (the oracle's 0 reads as dO).

    match: a local slot's value always moves by dO; a remote slot's moves when it holds something,
    that is when the oracle's value is non-zero or an ack reached the slot through this wrapper since
    the last become_leader / set_replicas (an ack of exactly dO leaves the oracle's 0)."""

    def __init__(self, ora, cfg, bases):
        self.ora, self.cfg = ora, cfg
        self.bases = {int(p): (int(o), int(q)) for p, (o, q) in bases.items()}
        for p, (_, dP) in self.bases.items():
            assert dP % cfg.index_interval == 0 and dP % 16 == 0, (p, dP)
        self._acked = set()
        self._rings = {}

    # ---- the translation (overridden by the deliberately wrong wrappers of the sensitivity check)
    def dO(self, p) -> int:
        return self.bases.get(int(p), (0, 0))[0]

    def dP(self, p) -> int:
        return self.bases.get(int(p), (0, 0))[1]

    def off_up(self, p, v) -> int:
        """An offset the engine reports for the oracle's v."""
        return int(v) + self.dO(p)

    def pos_up(self, p, v) -> int:
        return int(v) + self.dP(p)

    def stamp(self, p, v) -> int:
        """A record's header offset for the oracle's v."""
        return int(v) + self.dO(p)

    def off_down(self, p, v) -> int:
        d = int(v) - self.dO(p)
        if d < 0:
            raise ValueError(f"offset {v} of partition {p} lies below its base: it has no oracle counterpart")
        return d

    # ---- plumbing
    def close(self):
        self.ora.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __getattr__(self, name):  # whatever carries no offset or position (set_world, counters, ...)
        if name in ("ora", "cfg", "bases"):
            raise AttributeError(name)
        return getattr(self.ora, name)

    def _valid(self, p) -> bool:
        return 0 <= int(p) < self.cfg.num_partitions

    def _touch(self):
        self._rings.clear()

    # ---- control
    def become_leader(self, pidx, term):
        self._touch()
        self._acked = {k for k in self._acked if k[0] != int(pidx)}
        self.ora.become_leader(pidx, term)

    def set_replicas(self, pidx, ranks, leader_slot):
        self._touch()
        self._acked = {k for k in self._acked if k[0] != int(pidx)}
        self.ora.set_replicas(pidx, ranks, leader_slot)

    def set_segments(self, pidx, segment_bytes):
        self._touch()
        self.ora.set_segments(pidx, segment_bytes)

    def set_replica_cursor(self, pidx, offset):
        self.ora.set_replica_cursor(pidx, np.array([self.off_down(p, o) for p, o in zip(pidx, offset)], np.uint64))

    def ack(self, pidx, slot, match):
        self._touch()
        down = []
        for p, s, m in zip(pidx, slot, match):
            if self._valid(p):
                down.append(self.off_down(p, m))
                self._acked.add((int(p), int(s)))
            else:
                down.append(int(m))
        self.ora.ack(pidx, slot, np.array(down, np.uint64))

    # ---- append
    def append(self, pidx, lens, payload, payload_off=None):
        self._touch()
        out, st = self.ora.append(pidx, lens, payload, payload_off)
        up = [int(o) if int(o) == NONE else self.off_up(p, o) for p, o in zip(np.asarray(pidx).tolist(), out.tolist())]
        return np.array(up, np.uint64), st

    # ---- consumer offsets
    def commit_consumer_offset(self, pidx, consumer, offset):
        down = [self.off_down(p, o) if self._valid(p) else int(o) for p, o in zip(pidx, offset)]
        rc, st = self.ora.commit_consumer_offset(pidx, consumer, np.array(down, np.uint64))
        self.last_offset_ticket = self.ora.last_offset_ticket
        return rc, st

    def consumer_offsets(self, pidx):
        return np.array([self.off_up(pidx, v) for v in self.ora.consumer_offsets(pidx).tolist()], np.uint64)

    # ---- fetch
    def fetch(self, pidx, consumer, max_records, out_cap=None, commit=False, out=None, replica=False):
        rc, res, buf, used = self.ora.fetch(pidx, consumer, max_records, out_cap, commit=commit, out=out,
                                            replica=replica)
        return rc, self.fetch_up(pidx, res, buf), buf, used

    def fetch_up(self, pidx, res, buf):
        """The oracle's fetch rows and output (restamped in place) as the rebased engine answers."""
        res = res.copy()
        for r, p in enumerate(np.asarray(pidx).tolist()):
            if int(res["status"][r]) not in _MOVED or not self._valid(p):
                continue
            res["start_offset"][r] = self.off_up(p, res["start_offset"][r])
            nb = int(res["bytes"][r])
            if int(res["status"][r]) == A.RMQ_OK and nb and buf is not None:
                lo = int(res["out_pos"][r])
                restamp_records(buf[lo:lo + nb], lambda h, p=p: self.stamp(p, h))
        return res

    # ---- read-back
    def state(self, pidx):
        st = dict(self.ora.state(pidx))
        for f in OFFSET_FIELDS:
            st[f] = self.off_up(pidx, st[f])
        for f in POS_FIELDS:
            st[f] = self.pos_up(pidx, st[f])
        rank = self.cfg.rank
        st["match"] = [self.off_up(pidx, m) if (st["replica_rank"][r] == rank or m or (int(pidx), r) in self._acked)
                       else m for r, m in enumerate(st["match"])]
        return st

    def read_index(self, pidx, m_first, count):
        dm = self.dP(pidx) // self.cfg.index_interval
        if m_first < dm:
            raise ValueError(f"index entry {m_first} of partition {pidx} lies below its base")
        e = self.ora.read_index(pidx, m_first - dm, count)
        return np.array([(self.off_up(pidx, o), self.pos_up(pidx, q)) for o, q in e.tolist()], np.uint64).reshape(-1, 2)

    def _ring(self, replica, pidx):
        """The whole translated ring of one slot: the oracle's bytes rotated by dP mod S, and the
        header offset of every record of the retained window restamped (a walk over the window)."""
        key = (int(replica), int(pidx))
        if key in self._rings:
            return self._rings[key]
        st = self.ora.state(pidx)
        S, lo, hi = st["segment_bytes"], st["log_start_pos"], st["log_end_pos"]
        assert hi - lo <= S, st
        src = self.ora.read_segment(replica, pidx, 0, S)
        ring = np.empty(S, np.uint8)
        ring[(np.arange(S) + self.dP(pidx)) % S] = src
        n = st["log_end_offset"] - st["log_start_offset"]
        if n:
            win = src[(lo + np.arange(hi - lo)) % S]
            tab = record_positions(win, n, st["log_start_offset"])
            # a slot that is not local holds what it held when it left (a prefix of the window at
            # most): its windows are not comparable at a base, the tests pass local_slots
            if st["replica_rank"][int(replica)] == self.cfg.rank:
                assert len(tab) == n + 1 and int(tab[-1]) == hi - lo, (pidx, len(tab), n)
            for t in tab[:-1].tolist():
                h = int.from_bytes(win[t:t + 8].tobytes(), "little")
                at = (lo + t + self.dP(pidx)) % S  # headers are 16-byte aligned: they never wrap
                ring[at:at + 8] = np.frombuffer(self.stamp(pidx, h).to_bytes(8, "little"), np.uint8)
        self._rings[key] = ring
        return ring

    def read_segment(self, replica, pidx, ring_off=0, n=None):
        ring = self._ring(replica, pidx)
        n = ring.size - ring_off if n is None else n
        assert ring_off + n <= ring.size
        return ring[ring_off:ring_off + n].copy()


# ---- the deliberately wrong translations (CPU sensitivity check only)
class Truncated32(Translated):
    """Offsets and positions shifted by the low 32 bits of the base: what 32-bit arithmetic gives."""

    def dO(self, p):
        return super().dO(p) & 0xFFFFFFFF

    def dP(self, p):
        return super().dP(p) & 0xFFFFFFFF


class StampOffByOne(Translated):
    """Header offsets one record too high; everything else right."""

    def stamp(self, p, v):
        return super().stamp(p, v) + 1


class OffsetsOffByOne(Translated):
    """Every reported offset one too high; positions and header offsets right."""

    def off_up(self, p, v):
        return super().off_up(p, v) + 1


def rebase_oracle(ora, bases, lead_term=2):
    """The oracle's share of rebase(): rmq_become_leader alike."""
    for p in sorted(bases):
        ora.become_leader(p, lead_term)


# ---- scenarios (shared, so that the CPU file checks the preconditions of what the GPU file runs)
def scenario_batches(n=8, records=400, config_index=71):
    """Batches of `records` records of 0 B to 3,000 B (log-uniform: most are short, some pass the
    large-record path's 1 KiB) over the 8 partitions: about 20 KB per partition and batch, so 64 KiB
    rings wrap every third batch."""
    spec = StreamSpec(8, records, "uniform", size=(0, 3000), config_index=config_index)
    return [make_batch(spec, b) for b in range(n)]


def first_batch():
    """The batch that crosses the boundaries of bases_for(256): per partition 40 records of 0, 1, 17,
    33, 49 and 100 bytes by turns (16 to 128 bytes of log: the 37th offset and the byte 3 I fall
    inside the batch, the byte inside a record), then one of 1,500 bytes. The turns start where
    tests/test_high_base_model.py finds every edge reached, for I = 256 and I = 1024."""
    pidx, lens = [], []
    for j in range(41):
        for p in range(8):
            pidx.append(p)
            lens.append(1500 if j == 40 else (0, 1, 17, 33, 49, 100)[(j + 2 * p) % 6])
    rng = np.random.default_rng(7100)
    return Batch(np.array(pidx, np.uint32), np.array(lens, np.uint32), rng.integers(0, 256, sum(lens), dtype=np.uint8))


def window_records(eng, cfg, p, slot=0):
    """[(offset, logical position, payload length)] of partition p's retained window, from a plain
    walk over the bytes read back (engine, oracle or wrapper)."""
    from parity import ring_window

    st = eng.state(p)
    buf = ring_window(eng, cfg, slot, p, st)
    out, pos, off = [], 0, st["log_start_offset"]
    while pos < buf.size:
        h = int.from_bytes(buf[pos:pos + 8].tobytes(), "little")
        ln = int.from_bytes(buf[pos + 8:pos + 12].tobytes(), "little")
        assert h == off, (p, h, off)
        out.append((off, st["log_start_pos"] + pos, ln))
        pos += 16 + ((ln + 15) & ~15)
        off += 1
    assert off == st["log_end_offset"] and pos == buf.size
    return out


def _all(bases, consumer, add):
    """(pidx, consumer, offset) of one consumer of every partition at its base + add."""
    pp = np.arange(8, dtype=np.uint32)
    return pp, np.full(8, consumer, np.uint32), np.array([bases[int(p)][0] + add for p in pp], np.uint64)


def scenario_ops(bases, group=2):
    """The append scenario both files run: first_batch; consumer 0 to base + 5 and a fetch of 40 (the
    slice [5, 41) holds the 11th and the 37th record and the bytes I and 3 I); two batches; consumer 1 to base + 5;
    two more batches (the rings wrap, retention runs) and a fetch of consumer 1 (RMQ_EOFFSET) and of
    consumer 0 (served above the boundary); then pipelined launch groups of `group` batches with a
    fetch that commits after each."""
    b = scenario_batches(10)
    pp = np.arange(8, dtype=np.uint32)
    c0, c1 = np.zeros(8, np.uint32), np.ones(8, np.uint32)
    ops = [("append", first_batch()),
           ("consumer_commit",) + _all(bases, 0, 5), ("fetch", pp, c0, np.full(8, 40, np.uint32)),
           ("append", b[0]), ("append", b[1]),
           ("consumer_commit",) + _all(bases, 1, 5),
           ("append", b[2]), ("append", b[3]),
           ("fetch", pp, c1, np.full(8, 10, np.uint32)), ("fetch", pp, c0, np.full(8, 10, np.uint32))]
    rest = b[4:]
    for k in range(0, len(rest), group):
        ops.append(("pipelined", rest[k:k + group]))
        ops.append(("fetch", pp, c1, np.full(8, 40, np.uint32), None, True))
    return ops


def apply_ops(eng, ops, after=None):
    """The ops of parity.run_ops on one engine; after(op, result) is called after every step."""
    for op in ops:
        kind, res = op[0], None
        if kind == "append":
            res = eng.append(op[1].pidx, op[1].lens, op[1].payload)
        elif kind == "pipelined":
            res = [eng.append(b.pidx, b.lens, b.payload) for b in op[1]]
        elif kind == "consumer_commit":
            res = eng.commit_consumer_offset(*op[1:4])
        elif kind == "fetch":
            res = eng.fetch(op[1], op[2], op[3], op[4] if len(op) > 4 else None,
                            commit=bool(op[5]) if len(op) > 5 else False)
        elif kind in ("become_leader", "set_replicas", "set_segments", "ack"):
            res = getattr(eng, kind)(*op[1:])
        else:
            raise ValueError(kind)
        if after is not None:
            after(op, res)


def quorum_ops(bases):
    """Remote slots and acks on both sides of the boundaries (FORMAT.md §6): partitions 1, 5 and 3 keep
    slot 0 only (a quorum needs one ack), 2 keeps two slots; a new term; acks below and above 2^32,
    of exactly 2^31, far beyond the log end (clamped to it) and lower than the slot holds; a batch
    between them, and a fetch of a consumer that stands at the base (bounded by the high watermark)."""
    x, y = scenario_batches(2, config_index=73)
    o = {p: bases[p][0] for p in bases}
    pp = np.arange(8, dtype=np.uint32)
    ops = [("set_replicas", 1, [0, 1, 2], 0), ("set_replicas", 2, [0, 0, 1], 0), ("set_replicas", 5, [0, 1, 2], 0),
           ("set_replicas", 3, [0, 1, 0], 0)]
    ops += [("become_leader", p, 3) for p in (1, 2, 3, 5)]
    ops += [("append", x),
            ("ack", [1], [1], [o[1] + 10]),
            ("ack", [1, 1], [2, 1], [o[1] + 50, o[1] + 3]),
            ("ack", [2], [2], [o[2] + 2 ** 32]),
            ("ack", [5, 5], [1, 2], [o[5] + 7, o[5] + 10 ** 6]),
            ("ack", [3], [1], [o[3] + 11]),
            ("fetch", pp, np.full(8, 2, np.uint32), np.full(8, 1024, np.uint32)),
            ("append", y),
            ("ack", [1, 5, 3], [1, 1, 1], [2 ** 59, 2 ** 59 - 1, o[3] + 2 ** 31]),
            ("fetch", pp, np.full(8, 2, np.uint32), np.full(8, 1024, np.uint32))]
    return ops


def local_slots_of(eng):
    """local_slots for parity.run_ops / compare_state: the slots of p that this engine holds."""
    rank = eng.cfg.rank
    return lambda p: [r for r, x in enumerate(eng.state(p)["replica_rank"]) if x == rank]


# ---- a world of three ranks (tests/world_script.py), every rank rebased before it attaches
WORLD, PPR = 3, 2


def world_setup(I=256):
    """(views, cfgs, bases by rank {local pidx: base}): three ranks, two led partitions each, RF 3,
    32 KiB rings; global partition g starts at bases_for(I)[g] on every rank that holds it."""
    from repl_sim import rank_cfg
    from ripplemq_amd.sharding import rank_view

    views = [rank_view(r, WORLD, PPR, 3) for r in range(WORLD)]
    base = cfg_high(num_partitions=1, segment_bytes=1 << 15, index_interval=I, max_batch_bytes=1 << 18)
    cfgs = [rank_cfg(base, views[r], r) for r in range(WORLD)]
    B = bases_for(I)
    bases = [{p: B[int(g)] for p, g in enumerate(views[r].gp)} for r in range(WORLD)]
    return views, cfgs, bases


def world_steps(views, bases):
    """Term 3 on every leader, two rounds, a consumer commit on every leader (base + 30) and a fetch
    of 20, a round that rank 1 misses from rank 0, rounds that catch it up while the rings wrap, the
    fetch again (RMQ_EOFFSET by then), a last round.
    `bases` are those the offsets of the commits are written in ((0, 0) everywhere for the oracles)."""
    spec = StreamSpec(PPR, 80, "uniform", size=(0, 600), config_index=74)

    def rnd(k, faults=None):
        step = ("round", {r: [make_batch(spec, 1000 * r + 10 * k + j) for j in range(2)] for r in range(WORLD)})
        return step + (faults,) if faults else step

    led = np.arange(PPR, dtype=np.uint32)
    one = np.ones(PPR, np.uint32)
    commit = ("commit", {r: (led, one, np.array([bases[r][int(p)][0] + 30 for p in led], np.uint64)) for r in range(WORLD)})
    fetch = ("fetch", {r: (led, one, np.full(PPR, 20, np.uint32)) for r in range(WORLD)})
    return [("lead", {r: [(int(p), 3) for p in led] for r in range(WORLD)}), rnd(0), rnd(1), commit, fetch,
            rnd(2, {"lost": [(0, 1)]}), rnd(3), rnd(4), fetch, rnd(5)]


def follower_view(st, rank):
    """A state with what a follower does not maintain taken out: the match of the slots it does not
    hold, on a partition it does not lead (rmq_restore leaves the base there, a fresh log 0)."""
    st = dict(st)
    if not st["is_leader"]:
        st["match"] = [m if st["replica_rank"][r] == rank else None for r, m in enumerate(st["match"])]
    return st
