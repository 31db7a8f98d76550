"""Shared by tests/test_ingest_states.py (CPU) and tests/test_gpu_ingest_sweep.py: the follower-ingest
scenarios (FORMAT.md §9), a region parser written from FORMAT.md alone, the flip planner and the
lock-step drivers of the oracle and of the GPU engines. Every expected value of the GPU tests is the
oracle's (tests/repl_sim.py) or region_map's on the oracle's region; this module needs no GPU.

A scenario is rounds of one batch per rank with an rmq_sync after each, so the GPU engines plan every
round after the acks of the round before, as the oracle does: regions, counters and state are equal
bit for bit, round by round. A flip's byte position depends on the round's region, so the oracle
runs first with planners (callables on the parsed clean region); the positions it records drive
rmq_fault_corrupt on the GPU run, and the GPU's regions must equal the oracle's, flip included.
"""
from __future__ import annotations

import hashlib
import threading
from dataclasses import dataclass, field

import numpy as np

import scrub_util as U
from repl_sim import exchange_round, notice_round, place, rank_cfg
from ripplemq_amd.engine import EngineConfig
from ripplemq_amd.sharding import rank_view

HDR, DIR = 64, 48   # region header and directory entry bytes (FORMAT.md §9)
MAGIC = 0x34514D52
FLIP = 0x5A         # rmq_fault_corrupt's mask

# the length edges of the audit sweep plus the 4|5-piece edge of the verify's speculative loads
# (64 B is the last record loaded whole with its table slot, 65 B the first to enter the
# four-in-flight loop), and their neighbours one piece on
LENS_I = U.LENS3 + (63, 64, 65, 79, 80, 81)
PARTS_I = 4
FIELDS = ("off0", "off7", "len0", "crc0", "pay_first", "pay_last", "pad_first", "pad_last")
# scenario B: around one piece, the speculative-load edge, the apply stage's LDS image, the
# whole-wave threshold (64 pieces), 65 pieces with and without padding, two 1 KB strides, the largest
B_LENS = (0, 1, 16, 17, 64, 65, 112, 113, 1024, 1025, 1040, 1041, 4097, 16384)


def batch_i(b: int):
    """One cycle of LENS_I per partition, rotated per partition and batch, interleaved (as
    scrub_util.batch3): about 148 KB of records per partition."""
    rng = np.random.default_rng(5000 + b)
    pidx, lens = [], []
    for j in range(len(LENS_I)):
        for p in range(PARTS_I):
            pidx.append(p)
            lens.append(LENS_I[(j + p + b) % len(LENS_I)])
    payload = rng.integers(0, 256, sum(lens), dtype=np.uint8)
    return np.array(pidx, np.uint32), np.array(lens, np.uint32), payload


# ---- FORMAT.md §9: a region, parsed

def _u32(b, at):
    return int.from_bytes(bytes(b[at:at + 4]), "little")


def _u64(b, at):
    return int.from_bytes(bytes(b[at:at + 8]), "little")


def region_map(region) -> dict:
    """A round region by FORMAT.md §9: the header words, the directory entries, the table slots, the
    consumer-offset rows and, from a walk of every entry's bytes by the record headers (§1), the
    records: {"t": table index, "entry", "k": rank in the entry, "pos": byte position in the region,
    "len", "off": header offset}. The walk trusts only the directory's data_start and count; whether
    it agrees with the table and tiles the data section is for the caller to assert (check_map)."""
    b = np.ascontiguousarray(region, np.uint8)
    assert b.size >= HDR, b.size
    h = {"magic": _u32(b, 0), "n": _u32(b, 4), "N": _u32(b, 8), "src": _u32(b, 12), "keysum": _u64(b, 16),
         "data_off": _u64(b, 24), "rows_off": _u64(b, 32), "M": _u32(b, 40), "C": _u32(b, 44),
         "round": _u64(b, 48), "zero": _u64(b, 56), "size": int(b.size)}
    n, N = h["n"], h["N"]
    tab = HDR + DIR * n
    dirs = []
    for k in range(n):
        a = HDR + DIR * k
        dirs.append({"count": _u32(b, a), "bytes16": _u32(b, a + 4), "first": _u64(b, a + 8),
                     "tstart": _u32(b, a + 16), "dstart16": _u32(b, a + 20), "term": _u64(b, a + 24),
                     "commit": _u64(b, a + 32), "last_term": _u64(b, a + 40)})
    table = [(_u32(b, tab + 8 * t), _u32(b, tab + 8 * t + 4)) for t in range(N)]
    recs, t = [], 0
    for k, d in enumerate(dirs):
        pos = h["data_off"] + 16 * d["dstart16"]
        for j in range(d["count"]):
            ln = _u32(b, pos + 8)
            recs.append({"t": t, "entry": k, "k": j, "pos": pos, "len": ln, "off": _u64(b, pos)})
            pos += 16 + ((ln + 15) & ~15)
            t += 1
    rowb = 16 + 8 * h["C"]
    rows = [{"entry": _u32(b, h["rows_off"] + rowb * r), "pos": h["rows_off"] + rowb * r} for r in range(h["M"])]
    return {"hdr": h, "dir": dirs, "table": table, "recs": recs, "rows": rows, "tab_off": tab}


def rec_size(ln: int) -> int:
    return 16 + ((ln + 15) & ~15)


def check_map(m: dict) -> None:
    """The layout rules of FORMAT.md §9 on a parsed clean region: data_off and rows_off as defined,
    the records tile the data section exactly, the table slots agree with the walk."""
    h = m["hdr"]
    assert h["magic"] == MAGIC and h["zero"] == 0 and len(m["dir"]) == h["n"]
    assert h["data_off"] == HDR + DIR * h["n"] + ((8 * h["N"] + 15) & ~15), h
    assert len(m["recs"]) == h["N"] == sum(d["count"] for d in m["dir"])
    pos, t = h["data_off"], 0
    for k, d in enumerate(m["dir"]):
        assert d["tstart"] == t and h["data_off"] + 16 * d["dstart16"] == pos, (k, d)
        for j in range(d["count"]):
            r = m["recs"][t]
            assert (r["t"], r["entry"], r["k"], r["pos"], r["off"]) == (t, k, j, pos, d["first"] + j), (r, d)
            assert m["table"][t] == (k, (pos - h["data_off"]) // 16), (t, m["table"][t])
            pos += rec_size(r["len"])
            t += 1
        assert pos == h["data_off"] + 16 * (d["dstart16"] + d["bytes16"]), (k, d, pos)
    assert pos == h["rows_off"], (pos, h)  # rows_off = data_off + record bytes of all entries
    assert h["rows_off"] + len(m["rows"]) * (16 + 8 * h["C"]) == h["size"] and h["M"] <= h["n"]
    assert [r["entry"] for r in m["rows"]] == sorted({r["entry"] for r in m["rows"]})


def flip_positions(region, t: int, which=FIELDS, m: dict | None = None) -> dict:
    """{field: byte position in the region} of record t (table index) for the fields of `which` the
    record has: off0 / off7 the header offset's first and last byte, len0 and crc0 the first byte of
    its length and CRC words, pay_* its first and last payload byte, pad_* its first and last padding
    byte."""
    m = region_map(region) if m is None else m
    r = m["recs"][t]
    p, ln = r["pos"], r["len"]
    out = {"off0": p, "off7": p + 7, "len0": p + 8, "crc0": p + 12}
    if ln:
        out.update(pay_first=p + 16, pay_last=p + 16 + ln - 1)
    if ln % 16:
        out.update(pad_first=p + 16 + ln, pad_last=p + rec_size(ln) - 1)
    return {f: out[f] for f in which if f in out}


def field_at(m: dict, at: int):
    """(record, [fields]) of the region byte `at`, the inverse of flip_positions; (None, ["row_entry"])
    for the entry-index word of a consumer-offset row, (None, []) elsewhere."""
    for r in m["recs"]:
        if r["pos"] <= at < r["pos"] + rec_size(r["len"]):
            fp = flip_positions(None, r["t"], m=m)
            return r, [f for f in FIELDS if fp.get(f) == at]
    if any(w["pos"] <= at < w["pos"] + 4 for w in m["rows"]):
        return None, ["row_entry"]
    return None, []


# ---- scenarios

@dataclass
class Scenario:
    name: str
    world: int
    rf: int
    ppr: int
    rounds: int
    cfg: dict                    # EngineConfig fields shared by every rank
    batch: object                # (rank, round) -> (pidx, lens, payload): every rank appends one batch a round
    plans: dict = field(default_factory=dict)  # round -> [(src, dst, planner(region map) -> byte)]

    def views(self):
        return [rank_view(r, self.world, self.ppr, self.rf) for r in range(self.world)]

    def cfgs(self):
        base = EngineConfig(num_partitions=1, replication_factor=self.rf, pipeline_depth=1, **self.cfg)
        return [rank_cfg(base, v, r) for r, v in enumerate(self.views())]

    def pair_list(self, src: int, dst: int):
        """The entry list of the pair (FORMAT.md §9): (key, slot) of src's partitions with a slot on dst."""
        v = self.views()[src]
        return sorted((int(v.gp[p]), s) for p in range(v.led) for s in range(1, self.rf) if int(v.ranks[p][s]) == dst)


CFG_A = dict(segment_bytes=1 << 19, index_interval=1024, max_batch_records=1024, max_batch_bytes=1 << 20)


def _batch_a(r, k):
    return batch_i(7 * k + 3 * r)


def pick(entry=None, length=None, t=None, k=None, fld="pay_last", last=False, where=None):
    """A planner: the byte of field `fld` (the first that exists, of a tuple) of the last record of the
    clean region that matches entry / payload length / table index / rank in its entry (k = -1: the
    entry's last record) / where(record, directory entry)."""
    flds = (fld,) if isinstance(fld, str) else fld

    def plan(m):
        c = [r for r in m["recs"]
             if (entry is None or r["entry"] == entry) and (length is None or r["len"] == length) and
             (t is None or r["t"] == t) and
             (k is None or r["k"] == (k if k >= 0 else m["dir"][r["entry"]]["count"] + k)) and
             (where is None or where(r, m["dir"][r["entry"]]))]
        assert c, ("no such record", entry, length, t, k)
        fp = flip_positions(None, c[-1]["t"], m=m)
        return next(fp[f] for f in flds if f in fp)
    return plan


def row_entry_word(m):
    assert m["rows"], "the round carries no consumer-offset row"
    return m["rows"][0]["pos"]


def scenario_a() -> Scenario:
    return Scenario("A", 2, 2, PARTS_I, 5, CFG_A, _batch_a)


def b_lengths(fld: str):
    return [ln for ln in B_LENS if (ln or not fld.startswith("pa")) and (ln % 16 or not fld.startswith("pad"))]


def scenario_b(fld: str) -> Scenario:
    """One flip of field `fld` per round, rank 0 -> rank 1, in a record of each length of B_LENS that
    has the field; round k flips entry k mod 4, so the entry refused in round k - 1 is a catch-up
    entry of the region that carries the next flip. A last clean round lets every follower catch up."""
    lens = b_lengths(fld)
    plans = {k: [(0, 1, pick(entry=k % PARTS_I, length=ln, fld=fld))] for k, ln in enumerate(lens)}
    return Scenario("B-" + fld, 2, 2, PARTS_I, len(lens) + 1, CFG_A, _batch_a, plans)


NREC_I = len(LENS_I)  # records per partition and round in scenarios A and B


def _in_gap(r, d):
    # a catch-up entry carries the gap, re-read from the leader's ring, before the round's records
    return d["count"] > NREC_I and r["k"] < d["count"] - NREC_I and r["len"] > 1024


PLACES = ("tab63", "first_rec", "tab64", "last_rec", "gap", "big", "row_entry")


def scenario_b_places() -> Scenario:
    """Flips by place: table indices 63 and 64 (the last lane of a verify task and the first of the
    next), the first and the last record of an entry, the gap part of a catch-up entry, and the
    entry-index word of a consumer-offset row (a structural fault: the whole pair is refused)."""
    any_fld = ("pay_last", "crc0")
    plans = {
        0: [(0, 1, pick(t=63, fld=any_fld))],
        1: [(0, 1, pick(entry=1, k=0, fld=("pay_first", "crc0")))],
        2: [(0, 1, pick(t=64, fld=any_fld))],
        3: [(0, 1, pick(entry=2, k=-1, fld=("pad_last", "pay_last", "crc0")))],
        4: [(0, 1, pick(entry=2, where=_in_gap, fld="pay_last"))],   # entry 2 is refused twice
        5: [(0, 1, pick(entry=3, length=4097, fld="pay_first"))],    # (its catch-up gives round 6 a row)
        6: [(0, 1, row_entry_word)],
    }
    return Scenario("B-places", 2, 2, PARTS_I, 8, CFG_A, _batch_a, plans)


def scenario_b2() -> Scenario:
    """World 2, RF 3: rank 1 holds two slots of each of rank 0's partitions, entries 2p and 2p + 1."""
    plans = {0: [(0, 1, pick(entry=1, length=1025, fld="pay_last"))],
             1: [(0, 1, pick(entry=2, length=17, fld="pad_first"))]}
    return Scenario("B2", 2, 3, PARTS_I, 3, CFG_A, _batch_a, plans)


def scenario_b3() -> Scenario:
    """World 3, RF 3: in round 1 ranks 0 and 1 both send rank 2 a flipped region."""
    plans = {1: [(0, 2, pick(entry=0, length=17, fld="crc0")), (1, 2, pick(entry=2, length=4097, fld="pay_first"))]}
    return Scenario("B3", 3, 3, PARTS_I, 3, CFG_A, _batch_a, plans)


C_PARTS = 8
C_SIZES = (16368, 16384, 16400, 32768, 32784)
C_PAYLOADS = ([16352], [16368], [16384], [16384, 16352], [16384, 16368])


def _batch_c(r, k):
    rng = np.random.default_rng(6000 + 10 * k + r)
    if k == 0:  # partition p's log end at 16 p: phase p of the copy's 128-byte lines
        pidx = list(range(1, C_PARTS))
        lens = [16 * (p - 1) for p in pidx]
    else:
        pidx = [p for _ in C_PAYLOADS[k - 1] for p in range(C_PARTS)]
        lens = [ln for ln in C_PAYLOADS[k - 1] for _ in range(C_PARTS)]
    return np.array(pidx, np.uint32), np.array(lens, np.uint32), rng.integers(0, 256, sum(lens), dtype=np.uint8)


def scenario_c() -> Scenario:
    cfg = dict(segment_bytes=1 << 16, index_interval=1024, max_batch_records=1024, max_batch_bytes=1 << 20)
    return Scenario("C", 2, 2, C_PARTS, 1 + len(C_SIZES), cfg, _batch_c)


D_COUNTS = (1, 63, 64, 65, 128, 129)
D_CYCLE = (17, 1025, 100, 0, 33, 49, 65)


def d_rot(r, k):
    return 2 * k + 3 * r


def _batch_d(r, k):
    rng = np.random.default_rng(7000 + 10 * k + r)
    n = D_COUNTS[k]
    lens = [D_CYCLE[(i + d_rot(r, k)) % len(D_CYCLE)] for i in range(n)]
    return np.zeros(n, np.uint32), np.array(lens, np.uint32), rng.integers(0, 256, sum(lens), dtype=np.uint8)


def scenario_d() -> Scenario:
    cfg = dict(segment_bytes=1 << 17, index_interval=1024, max_batch_records=1024, max_batch_bytes=1 << 20)
    return Scenario("D", 3, 3, 1, len(D_COUNTS), cfg, _batch_d)


# ---- digests and runs

def digest(eng, cfg, view) -> dict:
    """What one rank holds after a round: the bulk states, the consumer offsets, the live index
    entries of every partition and a hash of the whole ring of every local replica slot."""
    st = eng.states()
    I = cfg.index_interval
    d = {"states": st, "cons": eng.consumer_table(), "index": {}, "rings": {}}
    for p in range(cfg.num_partitions):
        lo, hi = -(-int(st[p]["log_start_pos"]) // I), int(st[p]["log_end_pos"]) // I
        d["index"][p] = eng.read_index(p, lo, hi - lo + 1) if hi >= lo else np.zeros((0, 2), np.uint64)
        for s in range(cfg.replication_factor):
            if int(view.ranks[p][s]) == view.rank:
                d["rings"][(p, s)] = hashlib.blake2b(eng.read_segment(s, p).tobytes(), digest_size=16).hexdigest()
    return d


def digest_diff(a: dict, b: dict) -> list:
    """What differs between two digests of one rank: [(what, partition, slot or None)]."""
    out = []
    for p in range(len(a["states"])):
        if a["states"][p].tobytes() != b["states"][p].tobytes():
            out.append(("state", p, None))
        if not np.array_equal(a["cons"][p], b["cons"][p]):
            out.append(("consumer offsets", p, None))
        if not np.array_equal(a["index"][p], b["index"][p]):
            out.append(("index", p, None))
    out += [("ring", p, s) for (p, s), hx in a["rings"].items() if b["rings"].get((p, s)) != hx]
    return out


COUNTERS = ("records_ingested", "refused_crc", "refused_log", "bytes_ingested", "catchup_entries", "detached_plans")


@dataclass
class Run:
    regions: list = field(default_factory=list)   # [round][src][dst]: the region as sent (flip included)
    clean: list = field(default_factory=list)     # oracle only: the same before the flips
    flips: list = field(default_factory=list)     # [round]: [(src, dst, byte)]
    refused: list = field(default_factory=list)   # oracle only: [round]: {(src, dst): [entries refused]}
    counters: list = field(default_factory=list)  # [round][rank]: the six replication counters so far
    digests: list = field(default_factory=list)   # [round][rank]


def run_oracle(O, sc: Scenario, faults=True) -> Run:
    """The scenario on per-rank oracles. faults=True: the scenario's planners choose the flips (each
    is given region_map of its clean region); False: a clean run of the same batches."""
    views, cfgs = sc.views(), sc.cfgs()
    W = sc.world
    oras = [O.OracleEngine(c) for c in cfgs]
    run = Run()
    try:
        for r in range(W):
            place(oras[r], views[r], W)
        for k in range(sc.rounds):
            for r in range(W):
                b = sc.batch(r, k)
                _, st = oras[r].append(*b)
                assert st["appended"] == len(b[0]), (sc.name, k, r, st)
            cor = [(s, d, (lambda reg, pl=pl: pl(region_map(reg)))) for s, d, pl in sc.plans.get(k, ())] if faults else None
            trace = {}
            clean = exchange_round(oras, keep_regions=True, corrupt=cor, trace=trace)
            notice_round(oras)  # every round ends in an rmq_sync
            sent = [[None if x is None else x.copy() for x in row] for row in clean]
            for s, d, at in trace["flips"]:
                sent[s][d][at] ^= FLIP
            run.clean.append(clean)
            run.regions.append(sent)
            run.flips.append(list(trace["flips"]))
            run.refused.append({sd: [int(e) for e in np.flatnonzero((a[:, 0] >> np.uint64(62)) & np.uint64(1))]
                                for sd, a in trace["acks"].items()})
            run.counters.append([tuple(int(x) for x in oras[r].counters()) for r in range(W)])
            run.digests.append([digest(oras[r], cfgs[r], views[r]) for r in range(W)])
        return run
    finally:
        for o in oras:
            o.close()


def run_ranks(world, body, barrier=None, timeout=120):
    """body(rank) on a thread per rank, as each rank would be driven by its own process; the first
    failure is raised (a failing rank breaks the barrier, so the others do not wait for it)."""
    errs = [None] * world

    def wrap(r):
        try:
            body(r)
        except BaseException as ex:  # noqa: BLE001 - reported below
            errs[r] = ex
            if barrier is not None:
                barrier.abort()

    ts = [threading.Thread(target=wrap, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
        assert not t.is_alive(), "a rank hung"
    first = [r for r, ex in enumerate(errs) if ex is not None and not isinstance(ex, threading.BrokenBarrierError)]
    first = first or [r for r, ex in enumerate(errs) if ex is not None]
    if first:
        raise AssertionError(f"rank {first[0]}: {errs[first[0]]!r}") from errs[first[0]]


def run_gpu(sc: Scenario, flips) -> Run:
    """The scenario on GPU engines over the in-process transport, in lock step: every rank appends
    its batch, rmq_sync, a barrier, then records its outboxes, counters and digest. flips[k] =
    [(src, dst, byte)] of round k (the oracle run's record)."""
    from ripplemq_amd.engine import Engine, LocalHub
    views, cfgs = sc.views(), sc.cfgs()
    W = sc.world
    run = Run(regions=[[None] * W for _ in range(sc.rounds)], flips=[list(f) for f in flips],
              counters=[[None] * W for _ in range(sc.rounds)], digests=[[None] * W for _ in range(sc.rounds)])
    barrier = threading.Barrier(W)
    hub = LocalHub(W)
    engs = [Engine(c) for c in cfgs]
    try:
        def body(r):
            e = engs[r]
            e.attach_local(hub)
            place(e, views[r])
            for k in range(sc.rounds):
                for s, d, at in flips[k]:
                    if s == r:
                        e.fault_corrupt(d, at)
                e.append_async(*sc.batch(r, k))
                e.sync()
                barrier.wait(60)
                run.regions[k][r] = [e.read_outbox(d) if d != r else None for d in range(W)]
                st = e.replication_stats()
                run.counters[k][r] = tuple(st[c] for c in COUNTERS)
                run.digests[k][r] = digest(e, cfgs[r], views[r])

        run_ranks(W, body, barrier)
        return run
    finally:
        for e in engs:
            e.close()
        hub.close()


def compare_runs(sc: Scenario, gpu: Run, ora: Run) -> None:
    """Every round: the regions both ways (unmasked, the flipped byte included), the six replication
    counters, and every rank's digest, GPU against oracle."""
    for k in range(sc.rounds):
        for r in range(sc.world):
            for d in range(sc.world):
                want, got = ora.regions[k][r][d], gpu.regions[k][r][d]
                if d == r or want is None:
                    continue
                if not np.array_equal(got, want):
                    n = min(got.size, want.size)
                    bad = np.flatnonzero(got[:n] != want[:n])
                    raise AssertionError(f"{sc.name} round {k}: region {r}->{d} differs, sizes {got.size}/{want.size}, "
                                         f"first byte {bad[0] if bad.size else n}")
            assert gpu.counters[k][r] == ora.counters[k][r], \
                f"{sc.name} round {k} rank {r}: counters {COUNTERS} gpu={gpu.counters[k][r]} oracle={ora.counters[k][r]}"
            diff = digest_diff(gpu.digests[k][r], ora.digests[k][r])
            if diff:
                what, p, s = diff[0]
                raise AssertionError(f"{sc.name} round {k} rank {r}: {what} of partition {p}" +
                                     (f" slot {s}" if s is not None else "") + f" differs ({len(diff)} in all: {diff[:6]})")


def expected_refused(sc: Scenario, m: dict, src: int, dst: int, at: int) -> list:
    """The entries of the pair a flip of region byte `at` must refuse (FORMAT.md §9): the record's
    entry and the partition's other slot on the follower, or every entry for a structural fault."""
    rec, flds = field_at(m, at)
    pl = sc.pair_list(src, dst)
    assert len(pl) == m["hdr"]["n"]
    if rec is None:
        assert flds == ["row_entry"], (at, flds)
        return list(range(len(pl)))
    return [e for e in range(len(pl)) if pl[e][0] == pl[rec["entry"]][0]]
