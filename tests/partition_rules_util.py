"""The four partition rules of FORMAT.md §3-§6 (space rule, retention per batch, quorum commit with
its current-term gate, the rmq_ack clamp) as a small independent model, and the case tables that
tests/test_partition_rules_model.py (model against oracle, no GPU) and
tests/test_gpu_partition_rules.py (device against oracle and model) run.

PartitionModel restates FORMAT.md with Python ints, lists and dicts. It shares no code with oracle/
or ripplemq_amd/ and holds no payload bytes: ring and fetch contents stay the oracle's job.

Every table is deterministic, uses the smallest ring the engine takes (segment_bytes = 4096 =
4 * index_interval) and is a valid call sequence. Ops are tuples as tests/parity.py run_ops takes
them: ("append", batch), ("pipelined", [batch, ...]), ("ack", pidx, slot, match),
("become_leader", p, term), ("set_replicas", p, ranks, leader_slot).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ripplemq_amd.workload import Batch

S = 4096          # segment_bytes of every table
I = 256           # index_interval of every table
ROOM = S - I      # the most record bytes one batch may hold for one partition (FORMAT.md §3)
NONE = (1 << 64) - 1
ALL = 0xFFFFFFFF
MAX_BATCH = 4096

STATE_KEYS = ("log_end_offset", "log_end_pos", "log_start_offset", "log_start_pos", "commit",
              "high_watermark", "term", "term_start", "match", "is_leader", "segment_bytes")


def rec_size(length: int) -> int:
    return 16 + (length + 15) // 16 * 16


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------

class _Part:
    def __init__(self, rf: int, seg: int):
        self.leo = self.used = self.start_off = self.start_pos = 0
        self.E = {0: (0, 0)}
        self.match = [0] * rf
        self.commit = self.hw = 0
        self.term, self.term_start = 1, 0
        self.seg = seg
        self.local = [True] * rf  # every replica co-located at creation, led from term 1
        self.is_leader = True


class PartitionModel:
    """FORMAT.md §3-§6 for one engine of rank 0 without a transport."""

    def __init__(self, num_partitions: int, replication_factor: int, segment_bytes: int = S,
                 index_interval: int = I):
        self.P, self.RF, self.I = num_partitions, replication_factor, index_interval
        self.parts = [_Part(replication_factor, segment_bytes) for _ in range(num_partitions)]

    # §6: N = the k-th largest match, k = RF/2 + 1; commit = N if N > commit and N >= term_start
    def quorum_value(self, s: _Part) -> int:
        return sorted(s.match, reverse=True)[self.RF // 2]

    def _rule(self, s: _Part) -> None:
        n = self.quorum_value(s)
        if n > s.commit and n >= s.term_start:
            s.commit = n
        s.hw = s.commit

    # §4: once per append batch
    def _retain(self, s: _Part) -> None:
        if s.used - s.start_pos > s.seg:
            m = -(-(s.used - s.seg) // self.I)
            s.start_off, s.start_pos = s.E[m]

    def set_replicas(self, p: int, ranks, leader_slot: int) -> None:
        s = self.parts[p]
        s.local = [r == 0 for r in ranks]
        s.is_leader = s.is_leader and ranks[leader_slot] == 0  # a placement never starts a leadership

    def become_leader(self, p: int, term: int) -> None:
        for q in (range(self.P) if p == ALL else [p]):
            s = self.parts[q]
            assert any(s.local) and term > s.term
            s.is_leader, s.term, s.term_start = True, term, s.leo
            s.match = [s.leo if loc else 0 for loc in s.local]
            self._rule(s)

    def append(self, pidx, lens):
        """One batch (§3). Returns (out offsets, stats)."""
        st = dict(records=len(pidx), appended=0, rejected_not_leader=0, rejected_no_partition=0,
                  rejected_no_space=0, rejected_invalid=0)
        held = {}
        for p, n in zip(pidx, lens):
            if p < self.P:
                held[p] = held.get(p, 0) + rec_size(int(n))
        out, took = [], set()
        for p, n in zip(pidx, lens):
            p, n = int(p), int(n)
            if p >= self.P:
                st["rejected_no_partition"] += 1
                out.append(NONE)
                continue
            s = self.parts[p]
            if not s.is_leader:
                st["rejected_not_leader"] += 1
                out.append(NONE)
                continue
            if held[p] > s.seg - self.I:
                st["rejected_no_space"] += 1
                out.append(NONE)
                continue
            o, pos, rs = s.leo, s.used, rec_size(n)
            for m in range(pos // self.I + 1, (pos + rs) // self.I + 1):  # pos < m I <= pos + rs
                s.E[m] = (o + 1, pos + rs)
            s.leo, s.used = o + 1, pos + rs
            out.append(o)
            st["appended"] += 1
            took.add(p)
        for p in sorted(took):
            s = self.parts[p]
            s.match = [s.leo if loc else m for loc, m in zip(s.local, s.match)]
            self._rule(s)
            self._retain(s)
        return out, st

    def ack(self, pidx, slot, match) -> None:
        for p, r, m in zip(pidx, slot, match):
            s = self.parts[int(p)]
            s.match[int(r)] = max(s.match[int(r)], min(int(m), s.leo))
        for p in pidx:
            self._rule(self.parts[int(p)])

    def state(self, p: int) -> dict:
        s = self.parts[p]
        return {"log_end_offset": s.leo, "log_end_pos": s.used, "log_start_offset": s.start_off,
                "log_start_pos": s.start_pos, "commit": s.commit, "high_watermark": s.hw, "term": s.term,
                "term_start": s.term_start, "match": list(s.match), "is_leader": int(s.is_leader),
                "segment_bytes": s.seg}

    def live_index(self, p: int):
        """(first live m, [[offset, pos], ...]) of §5's live range (empty list: none live)."""
        s = self.parts[p]
        lo, hi = -(-s.start_pos // self.I), s.used // self.I
        return lo, [list(s.E[m]) for m in range(lo, hi + 1)]

    def apply(self, op):
        """One op of a table. Returns [(out offsets, stats)] of its batches."""
        kind = op[0]
        if kind == "append":
            return [self.append(op[1].pidx, op[1].lens)]
        if kind == "pipelined":
            return [self.append(b.pidx, b.lens) for b in op[1]]
        if kind == "ack":
            self.ack(op[1], op[2], op[3])
        elif kind == "become_leader":
            self.become_leader(op[1], op[2])
        elif kind == "set_replicas":
            self.set_replicas(op[1], op[2], op[3])
        elif kind == "set_placement":
            for p, ranks, slot in zip(op[1], op[2], op[3]):
                self.set_replicas(p, ranks, slot)
        else:
            raise ValueError(kind)
        return []


def engine_view(eng, p: int) -> dict:
    """The words of an engine's (device or oracle) state that the model keeps."""
    st = eng.state(p)
    return {k: st[k] for k in STATE_KEYS}


def assert_model_agrees(model: PartitionModel, eng, parts, who: str) -> None:
    for p in parts:
        want, got = model.state(p), engine_view(eng, p)
        assert got == want, f"partition {p}: {who} and the model differ\n {who}={got}\n model={want}"
        lo, ent = model.live_index(p)
        if ent:
            idx = eng.read_index(p, lo, len(ent)).tolist()
            assert idx == ent, f"partition {p}: live index from m={lo}\n {who}={idx}\n model={ent}"


def apply_oracle(ora, op):
    """One op of a table on the oracle alone. Returns [(out offsets, stats)] of its batches."""
    kind = op[0]
    if kind == "append":
        return [ora.append(op[1].pidx, op[1].lens, op[1].payload)]
    if kind == "pipelined":
        return [ora.append(b.pidx, b.lens, b.payload) for b in op[1]]
    if kind == "ack":
        ora.ack(op[1], op[2], op[3])
    elif kind == "become_leader":
        ora.become_leader(op[1], op[2])
    elif kind == "set_replicas":
        ora.set_replicas(op[1], op[2], op[3])
    elif kind == "set_placement":
        ora.set_placement(op[1], None, op[2], op[3])
    else:
        raise ValueError(kind)
    return []


# ------------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------------

def mk_batch(recs) -> Batch:
    """A batch of (partition, payload length) records in that order, payload bytes by position."""
    pidx = np.array([p for p, _ in recs], np.uint32)
    lens = np.array([n for _, n in recs], np.uint32)
    total = int(lens.sum())
    payload = ((np.arange(total, dtype=np.uint64) * 7 + len(recs)) & 255).astype(np.uint8)
    return Batch(pidx, lens, payload)


def interleave(a, b):
    """Records of a and b alternating, record by record, the longer list's tail last."""
    out = []
    for k in range(max(len(a), len(b))):
        out += a[k:k + 1] + b[k:k + 1]
    return out


def equal_records(p: int, total: int, rs: int):
    """Records of rs bytes each for p, `total` bytes; a tail of 16-byte pieces where rs does not divide."""
    assert total % 16 == 0 and rs % 16 == 0 and rs >= 16
    recs = [(p, rs - 16)] * (total // rs)
    rest = total - rs * len(recs)
    if rest:
        recs.append((p, rest - 16))
    return recs


UNEQUAL = (0, 1, 16, 17, 100, 0, 33, 250, 15, 0, 64, 7)  # payload lengths, zero-length ones included


def unequal_records(p: int, total: int):
    """Records of unequal sizes for p that sum to `total` bytes exactly."""
    recs, left, k = [], total, 0
    while left:
        rs = rec_size(UNEQUAL[k % len(UNEQUAL)])
        k += 1
        if rs > left:
            recs.append((p, left - 16))
            break
        recs.append((p, UNEQUAL[(k - 1) % len(UNEQUAL)]))
        left -= rs
    assert sum(rec_size(n) for _, n in recs) == total
    return recs


def bytes_for(batch: Batch, p: int) -> int:
    return sum(rec_size(int(n)) for q, n in zip(batch.pidx, batch.lens) if q == p)


def small(q: int, n: int = 3, length: int = 5):
    return [(q, length + k) for k in range(n)]


@dataclass
class Table:
    name: str
    cfg: dict                       # EngineConfig keywords
    ops: list
    local: dict = field(default_factory=dict)  # partition -> its local replica slots (default: all)
    notes: dict = field(default_factory=dict)  # what the model test must find, by the table's own words

    def local_slots(self, p):
        return self.local.get(p, range(self.cfg["replication_factor"]))


def base_cfg(P: int, RF: int, G: int = 2) -> dict:
    return dict(num_partitions=P, replication_factor=RF, segment_bytes=S, index_interval=I,
                max_consumers=2, max_batch_records=MAX_BATCH, pipeline_depth=G)


# ------------------------------------------------------------------------------------------------
# A. commit rule, every RF
# ------------------------------------------------------------------------------------------------

def masks_for(RF: int):
    """Local-slot masks of table A: slot 0 only, the highest slot only, k - 1 slots, k slots that are
    not contiguous, all slots; duplicates and the empty mask dropped."""
    k = RF // 2 + 1
    cand = [[0], [RF - 1], list(range(k - 1)), [0] + list(range(RF - k + 1, RF)), list(range(RF))]
    out = []
    for m in cand:
        m = sorted(set(m))
        if m and m not in out:
            out.append(m)
    return out


def ranks_of(mask, RF: int):
    """Local slots have rank 0, remote slot r has rank r + 1."""
    return [0 if r in mask else r + 1 for r in range(RF)]


WALK = (5, 9, 3, 8, 4, 7, 6)  # the values the remote slots are walked up with, in slot order
LONG_ACK_ITEMS = 1200         # past the 1024-item control area and four blocks of 256 threads
SEED_A = 20240611


def table_a(RF: int) -> Table:
    masks = masks_for(RF)
    P = len(masks)
    remote = [[r for r in range(RF) if r not in m] for m in masks]
    ops, notes = [], {}

    def ack(items):
        if items:
            ops.append(("ack", [i[0] for i in items], [i[1] for i in items], [i[2] for i in items]))
        return len(ops) - 1 if items else None

    def every(records):
        return mk_batch([rec for k in range(records) for p in range(P) for rec in [(p, (7 * k + 3 * p) % 41)]])

    for p, m in enumerate(masks):
        ops.append(("set_replicas", p, ranks_of(m, RF), m[0]))
    for p in range(P):
        ops.append(("become_leader", p, 2))
    ops.append(("append", every(20)))  # log end 20 everywhere
    leo = 20
    # a follower that holds nothing yet, then the remote slots one at a time with distinct values
    notes["zero"] = ack([(p, remote[p][0], 0) for p in range(P) if remote[p]])
    notes["walk"] = [ack([(p, remote[p][i], WALK[i]) for p in range(P) if i < len(remote[p])])
                     for i in range(max((len(r) for r in remote), default=0))]
    notes["no_regress"] = ack([(p, r, 1) for p in range(P) for r in remote[p]])
    notes["clamp"] = ack([(p, remote[p][0], 10 ** 12) for p in range(P) if remote[p]])
    notes["local_low"] = ack([(p, masks[p][0], 1) for p in range(P)])
    notes["local_high"] = ack([(p, masks[p][0], 10 ** 6) for p in range(P)])
    # one (partition, slot) three times in one call, in two orders: the maximum wins
    dup = [(p, remote[p][-1] if remote[p] else 0) for p in range(P)]
    notes["dup"] = [ack([(p, r, v) for p, r in dup for v in (11, 13, 12)]),
                    ack([(p, r, v) for v in (16, 14, 15) for p, r in dup])]
    # the long call: every (partition, slot) many times, values and order shuffled; even slots also
    # get values above the log end (clamped), odd slots stay below it
    g = np.random.default_rng(SEED_A + RF)
    pairs = [(p, r) for p in range(P) for r in range(RF)]
    items = []
    for i in range(LONG_ACK_ITEMS):
        p, r = pairs[i % len(pairs)]
        items.append((p, r, int(g.integers(0, leo + 4 if r % 2 == 0 else leo - 2))))
    order = g.permutation(len(items))
    notes["long"] = ack([items[i] for i in order])
    # records of term 2 that only a local quorum commits, then the next term
    ops.append(("append", every(6)))
    leo += 6
    notes["term3"] = len(ops)
    for p in range(P):
        ops.append(("become_leader", p, 3))
    notes["gate_below"] = ack([(p, r, leo - 1) for p in range(P) for r in remote[p]])
    notes["gate_first"] = ack([(p, remote[p][0], leo) for p in range(P) if remote[p]])
    notes["gate_at"] = ack([(p, r, leo) for p in range(P) for r in remote[p]])
    # back-to-back submissions (launch groups of pipeline_depth 2) with acks between the groups
    ops.append(("pipelined", [every(3), every(2)]))
    leo += 5
    ack([(p, r, leo - 1 - i) for p in range(P) for i, r in enumerate(remote[p])])
    ops.append(("pipelined", [every(2), every(3), every(1)]))
    leo += 6
    notes["last"] = ack([(p, r, leo) for p in range(P) for r in remote[p][::2]])
    notes.update(masks=masks, remote=remote, leo=leo)
    return Table(f"A-rf{RF}", base_cfg(P, RF, 2), ops, {p: m for p, m in enumerate(masks)}, notes)


# ------------------------------------------------------------------------------------------------
# B. space rule: p = 0 interleaved record by record with q = 1
# ------------------------------------------------------------------------------------------------

def table_b() -> Table:
    p, q = 0, 1
    fit_eq = equal_records(p, ROOM, 48)
    fit_un = unequal_records(p, ROOM)
    over_eq = fit_eq + [(p, 0)]            # one more zero-length record: 16 bytes over
    over_un = fit_un[:7] + [(p, 0)] + fit_un[7:]

    def with_q(recs):
        return mk_batch(interleave(recs, [(q, k % 23) for k in range(len(recs))]))

    names = ["fit_equal", "over_equal", "fit_unequal", "over_unequal", "fit_equal_wrapped", "over_equal_wrapped",
             "fit_unequal_wrapped", "over_unequal_wrapped"]
    recs = [fit_eq, over_eq, fit_un, over_un, fit_eq, over_eq, fit_un, over_un]
    ops = [("append", with_q(r)) for r in recs]
    return Table("B", base_cfg(2, 2), ops, notes={"names": names, "p": p, "q": q})


# ------------------------------------------------------------------------------------------------
# C. retention threshold
# ------------------------------------------------------------------------------------------------

def table_c() -> Table:
    """Partitions: 0 threshold walk (48-byte records, entries straddled), 1 and 2 the two sides of the
    ceil with 64-byte records (entries exactly on m I), 3 the same with 48-byte records, 4 and 5 the
    split pair."""
    ops, notes = [], {}

    def one(p, total, rs=48):
        ops.append(("append", mk_batch(equal_records(p, total, rs))))
        return len(ops) - 1

    # 0: end - start == S exactly (no move), then 16 bytes (move to E[1]); again from the moved start
    one(0, ROOM)
    notes["full0"] = one(0, I)               # 3840 + 256 = 4096 = S
    notes["move0"] = one(0, 16)              # E[1] = (6, 288): a record straddles 256
    notes["full1"] = one(0, 288 + S - 4112)  # end - 288 == S
    notes["move1"] = one(0, 16)              # m* = ceil(304 / 256) = 2
    # 1 / 2: log_end_pos - S == I exactly, and that plus 16
    for p, extra in ((1, 0), (2, 16)):
        one(p, ROOM, 64)
        notes[f"ceil{p}"] = one(p, 2 * I + extra, 64)
    for p, extra in ((3, 0),):
        one(p, ROOM, 48)
        notes[f"ceil{p}"] = one(p, 2 * I + extra, 48)
    # 4 / 5: the same records cut into batches at different places. Partition 4: 3840, then 512 and 32
    # in one launch group (after 512 the end is S + 256 and the start moves to E[1].pos = 288; after 32
    # more, end - start == S: no move). Partition 5: 3840, then 544 in one batch: m* = 2.
    head = equal_records(4, ROOM, 48)
    mid = equal_records(4, 480, 48) + [(4, 16)]
    tail = [(4, 16)]
    ops.append(("append", mk_batch(head)))
    ops.append(("pipelined", [mk_batch(mid), mk_batch(tail)]))
    notes["split_a"] = len(ops) - 1
    to5 = lambda recs: [(5, n) for _, n in recs]
    ops.append(("append", mk_batch(to5(head))))
    ops.append(("append", mk_batch(to5(mid + tail))))
    notes["split_b"] = len(ops) - 1
    return Table("C", base_cfg(6, 2), ops, notes=notes)


def table_c_split() -> Table:
    """The split pair of table C alone (its last four ops)."""
    t = table_c()
    return Table("C-split", t.cfg, t.ops[-4:], notes={"split_a": 1, "split_b": 3})


# ------------------------------------------------------------------------------------------------
# D. launch groups and the late path: p = 0, q = 1
# ------------------------------------------------------------------------------------------------

DEPTHS = (1, 2, 3, 8)
ORDERS = ("read", "sync", "next_with_p", "next_without_p")
D_CASES = ("two_full", "pair_at_ring", "pair_past_room", "pair_past_ring", "g_full", "middle_empty",
           "middle_refused", "not_led")
P_D, Q_D = 0, 1


@dataclass
class GroupCase:
    name: str
    G: int
    pre: list        # ops applied and drained before the case's batches
    batches: list    # submitted back to back
    led: bool = True


def _pq(p_bytes: int, k: int, rs: int = 64):
    """A batch with p_bytes for p (rs-byte records) interleaved with a few records of q."""
    return mk_batch(interleave(equal_records(P_D, p_bytes, rs) if p_bytes else [], small(Q_D, 3, 5 + k)))


def group_case(name: str, G: int) -> GroupCase:
    if name == "two_full":        # the smallest late case: ceil((fin_2 - S) / I) I > used0
        return GroupCase(name, G, [], [_pq(ROOM, 0), _pq(ROOM, 1)])
    if name.startswith("pair_"):  # used0 = 1024, a multiple of I; two batches add X together
        X = {"pair_at_ring": S, "pair_past_room": ROOM + 16, "pair_past_ring": S + 16}[name]
        a = X // 32 * 16
        return GroupCase(name, G, [("append", _pq(4 * I, 9))], [_pq(a, 0, 16), _pq(X - a, 1, 16)])
    if name == "g_full":          # G batches of S - I: with G = 8, seven and a half rings in one launch
        return GroupCase(name, G, [], [_pq(ROOM, k) for k in range(G)])
    if name == "middle_empty":
        return GroupCase(name, G, [], [_pq(ROOM, 0), _pq(0, 1), _pq(ROOM, 2)])
    if name == "middle_refused":
        return GroupCase(name, G, [], [_pq(ROOM, 0), _pq(ROOM + 16, 1, 16), _pq(ROOM, 2)])
    if name == "not_led":         # p's replica here follows rank 1; q is led
        return GroupCase(name, G, [("set_replicas", P_D, [1, 0, 2], 0)], [_pq(ROOM, 0), _pq(ROOM, 1)], led=False)
    raise ValueError(name)


def further_batches(case: GroupCase, order: str):
    """What follows the case's batches before anything is waited for.
    read: fillers of q alone until the case's last group and two more groups are closed, so that the
    launch applying the case's last group has been issued when the state is read;
    next_*: the rest of the case's last group and one whole group more, adding to p or not."""
    n, G = len(case.batches), case.G
    groups = -(-n // G)
    if order == "sync":
        return []
    if order == "read":
        return [_pq(0, 20 + k) for k in range((groups + 2) * G - n)]
    add = 64 if order == "next_with_p" else 0
    return [_pq(add, 40 + k) for k in range((groups + 1) * G - n)]


def late_batches(case: GroupCase, extra=()):
    """By §4 and the launch's read limit alone, nothing run: for the case's batches followed by
    `extra`, cut into launch groups of G, the indexes of the batches whose retention the launch
    applying them cannot finish. A launch reads only index entries at positions <= used0, the log
    end before its group; batch j needs entry m* = ceil((fin_j - S) / I) when fin_j - start > S; the
    first batch with m* I > used0 stops the replay, and it and every later batch of the group that
    still moves the start are late. Returns (late indexes, indexes of batches that move the start)."""
    model = PartitionModel(2, 3)
    for op in case.pre:
        model.apply(op)
    batches = list(case.batches) + list(extra)
    late, moved = [], []
    for g0 in range(0, len(batches), case.G):
        used0 = model.parts[P_D].used
        stopped = False
        for j in range(g0, min(g0 + case.G, len(batches))):
            s = model.parts[P_D]
            before = (s.used, s.start_pos)
            model.append(batches[j].pidx, batches[j].lens)
            if s.used == before[0] or s.used - before[1] <= S:
                continue  # added nothing to p, or no move
            moved.append(j)
            if stopped or -(-(s.used - S) // I) * I > used0:
                stopped = True
                late.append(j)
    return late, moved


def table_d(name: str, G: int, order: str) -> Table:
    case = group_case(name, G)
    ops = list(case.pre) + [("pipelined", list(case.batches) + further_batches(case, order))]
    return Table(f"D-{name}-G{G}-{order}", base_cfg(2, 3, G), ops, notes={"case": case})


# ------------------------------------------------------------------------------------------------
# E. reads and leader start over many partitions
# ------------------------------------------------------------------------------------------------

P_E, RF_E = 600, 8
E_RANGES = ((0, 600), (255, 2), (256, 344), (599, 1))
E_MASKS = ([0], [7], [0, 1, 2, 3], [0, 4, 5, 6, 7], list(range(8)), [2, 5], [1, 3, 4, 6, 7])


def mask_e(p: int):
    return E_MASKS[(p + p // 7) % len(E_MASKS)]


def table_e() -> Table:
    """ops: ("set_placement", pidx, ranks, leader_slot) first (one call for all 600 partitions)."""
    P, RF = P_E, RF_E
    ranks = [ranks_of(mask_e(p), RF) for p in range(P)]
    ops = [("set_placement", list(range(P)), ranks, [mask_e(p)[0] for p in range(P)]),
           ("become_leader", ALL, 2),
           ("append", mk_batch([(p, (p * 5 + k) % 30) for k in range(3) for p in range(P) if k < 1 + p % 3]))]
    g = np.random.default_rng(SEED_A)
    n = 1500
    pp = g.integers(0, P, n)
    ops.append(("ack", pp.tolist(), g.integers(0, RF, n).tolist(), g.integers(0, 5, n).tolist()))
    ops.append(("append", mk_batch([(p, (p * 3) % 17) for p in range(0, P, 2)])))
    ops.append(("become_leader", ALL, 3))
    pp = g.integers(0, P, n)
    ops.append(("ack", pp.tolist(), g.integers(0, RF, n).tolist(), g.integers(0, 6, n).tolist()))
    ops.append(("append", mk_batch([(p, 9) for p in range(0, P, 3)])))
    return Table("E", base_cfg(P, RF), ops, {p: mask_e(p) for p in range(P)})
