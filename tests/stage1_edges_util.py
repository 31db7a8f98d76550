"""Stage 1 of the append pipeline (pipeline.hip: stage1_tile, stage1_tile_hash) at the edges of its
tile, its 64-record slots and waves, its key widths and its hash table: the case tables, and an
independent model of what stage 1 is specified to produce for a tile.

Stage 1 gives every record its stable rank and its bytes/16 prefix inside its (tile, partition) run
and writes one cell {records, bytes/16} per (tile, partition) that holds a valid record. The sort
mode (RMQ_RANK unset) sorts the tile's 1024 items by key (the partition; 0 for records of unknown
partitions and for the junk lanes past the batch's last record) and scans the sorted items in waves
of 64-lane slots; the hash mode (RMQ_RANK=1) serves the 64-record slots of the input in order against
counters in an LDS hash table of 2048 slots. The kernel is built twice: 256 threads (4 waves, 256
sorted items a wave) for an engine alone and 512 threads (8 waves, 128 items a wave) for an engine
with a replication transport, so a wave boundary sits at other positions in the two.

The model restates, with numpy and Python ints and no code of ripplemq_amd/csrc or oracle/:
  record_flags   which records stage 1 flags (unknown partition, bad explicit payload range);
  tile_model     per tile: rank and bytes/16 prefix of each valid record, the cells, the large
                 records, the payload prefix;
  sorted_runs    the runs of equal keys of a tile in the sort mode's order, junk lanes included;
  run_edges      what a tile's runs are to the slot and wave boundaries of a geometry;
  hash_slot      h of stage1_tile_hash; probe_tile: its probe sequence over a 2048-slot table.

tests/test_stage1_edges_model.py proves on the CPU that every table holds the edge it is named for,
in both geometries, and that the C oracle agrees with the model; tests/test_gpu_stage1_edges.py runs
the tables on the device in both modes and through both kernels.

A table is a list of groups; a group is a list of device_batch_util.Case (a workload Batch, and for
explicit payload offsets `poff`, `declared` and `invalid`) submitted before any is waited for.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from device_batch_util import Case
from ripplemq_amd.workload import Batch

TILE_RECS = 1024     # kTileRecs: records per stage-1 tile
SLOT = 64            # records of one wave instruction: a slot
WAVE_RECS = {"single": 256, "transport": 128}  # kWR: sorted items per wave, 256- and 512-thread kernel
HT = 2048            # kHT: slots of stage1_tile_hash's table
BIG_LEN = 1024       # records of more payload bytes go to the large-record list (16 * kBigPieces)
FL_NOPART, FL_INVALID = 1, 4  # kFlNoPart, kFlInvalid
MIB = 1 << 20
NONE = (1 << 64) - 1
UNKNOWN = 0xFFFFFFFF  # a partition index no engine has


def _rng(tag: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[0x53314544, tag]))  # "S1ED"


def tiles_of(n: int) -> int:
    return -(-n // TILE_RECS)


# ------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------

def key_width(P: int) -> tuple[int, int]:
    """(key_bits, key_passes) of an engine of P partitions: the bits of P - 1, and the 8-bit radix
    passes that sort them (none for a single partition)."""
    bits = (P - 1).bit_length()
    return bits, 0 if bits == 0 else 1 if bits <= 8 else 2


def units(lens) -> np.ndarray:
    """16-byte units of each record as stored: the header and the payload padded to 16."""
    return 1 + (np.asarray(lens, np.int64) + 15) // 16


def declared_bytes(c: Case) -> int:
    return int(c.batch.payload.size if c.declared is None else c.declared)


def record_flags(c: Case, P: int):
    """(flags[n], records with a bad payload range). A record of partition >= P is FL_NOPART. With
    explicit offsets a record of L > 0 bytes at o is out of range when o > D or L > D - o (D: the
    declared payload bytes); it is counted, and flagged FL_INVALID unless it is FL_NOPART already.
    One counted record rejects the whole batch (stage 2's rule)."""
    b = c.batch
    fl = np.where(b.pidx.astype(np.int64) >= P, FL_NOPART, 0)
    bad = 0
    if c.poff is not None:
        D = declared_bytes(c)
        for k, (o, L) in enumerate(zip(c.poff.tolist(), b.lens.tolist())):
            if L and (o > D or L > D - o):
                bad += 1
                if not fl[k]:
                    fl[k] = FL_INVALID
    return fl, bad


@dataclass
class TileModel:
    nin: int            # records of the tile
    key: np.ndarray     # [nin] the key stage 1 sorts / hashes by: the partition, 0 for FL_NOPART
    fl: np.ndarray      # [nin]
    rank: np.ndarray    # [nin] valid records before it in its (tile, partition) run (valid records only)
    pre16: np.ndarray   # [nin] and their 16-byte units
    cells: dict         # partition -> (valid records, their units); no entry without a valid record
    big: list           # tile positions of the valid records of more than 1024 payload bytes
    pre: np.ndarray     # [nin] payload bytes of the tile's earlier records, flagged ones included


def tile_model(c: Case, P: int, t: int, fl=None) -> TileModel:
    b = c.batch
    fl = record_flags(c, P)[0] if fl is None else fl
    lo, hi = t * TILE_RECS, min((t + 1) * TILE_RECS, b.n)
    pidx, lens, f = b.pidx[lo:hi].astype(np.int64), b.lens[lo:hi].astype(np.int64), fl[lo:hi]
    u = units(lens)
    rank, pre16 = np.zeros(hi - lo, np.int64), np.zeros(hi - lo, np.int64)
    cells, big = {}, []
    for q in range(hi - lo):
        if f[q]:
            continue
        n, s = cells.get(int(pidx[q]), (0, 0))
        rank[q], pre16[q] = n, s
        cells[int(pidx[q])] = (n + 1, s + int(u[q]))
        if lens[q] > BIG_LEN:
            big.append(q)
    pre = np.concatenate([[0], np.cumsum(lens)[:-1]]) if hi > lo else np.zeros(0, np.int64)
    return TileModel(hi - lo, np.where(f == FL_NOPART, 0, pidx), f, rank, pre16, cells, big, pre)


def sorted_runs(tm: TileModel) -> list:
    """[(key, start, end, valid records)] of the tile's 1024 items in the sort mode's order: by key,
    equal keys in input order; the junk lanes (key 0, positions >= nin) end key 0's run."""
    key = np.zeros(TILE_RECS, np.int64)
    key[:tm.nin] = tm.key
    valid = np.zeros(TILE_RECS, bool)
    valid[:tm.nin] = tm.fl == 0
    order = np.argsort(key, kind="stable")
    ks = key[order]
    cut = [0] + (np.flatnonzero(ks[1:] != ks[:-1]) + 1).tolist() + [TILE_RECS]
    return [(int(ks[a]), a, b, int(valid[order[a:b]].sum())) for a, b in zip(cut[:-1], cut[1:])]


def run_edges(runs, wave_recs: int) -> set:
    """What the runs [(key, start, end, ...)] of one sorted tile are to the slots (64 items) and the
    waves (wave_recs items) of the segmented scan."""
    out = set()
    heads = [r[1] for r in runs]
    for _, a, b, *_ in runs:
        if a % SLOT == SLOT - 1:
            out.add("starts_at_lane_63")
        if (b - 1) % SLOT == 0 and b - 1 > a:
            out.add("ends_at_lane_0")
        if b - a == TILE_RECS:
            out.add("whole_tile")
        if a // SLOT != (b - 1) // SLOT and a // wave_recs == (b - 1) // wave_recs:
            out.add("crosses_slot_in_wave")   # carried by `carry` / hb
        if a // wave_recs != (b - 1) // wave_recs:
            out.add("crosses_wave")           # carried by wtail / the cin loop
        if b // wave_recs - (a // wave_recs + 1) >= 2:
            out.add("two_whole_waves_without_head")  # the cin loop walks back over both
        if b - a == 1:
            out.add("single_item_run")
    for w in range(TILE_RECS // wave_recs):
        hw = [h for h in heads if w * wave_recs <= h < (w + 1) * wave_recs]
        if hw and min(hw) >= (w + 1) * wave_recs - SLOT:
            out.add("head_only_in_last_slot_of_wave")
        if hw and max(hw) < w * wave_recs + SLOT and wave_recs > SLOT:
            out.add("head_only_in_first_slot_of_wave")
    if len(runs) == TILE_RECS:
        out.add("every_item_a_head")
    return out


def hash_slot(p) -> np.ndarray:
    """h of a partition, as read from stage1_tile_hash: kv = p + 1, h = (kv * 2654435761 mod 2^32)
    >> (32 - 11): the first of the table's 2048 slots the partition's leader looks at; every further
    look is at (h + 1) & 2047."""
    kv = (np.asarray(p, np.uint64) + np.uint64(1)) & np.uint64(0xFFFFFFFF)
    return (((kv * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(21)).astype(np.int64)


def probe_tile(tm: TileModel) -> dict:
    """The hash mode's table over one tile: the 64-record slots of the input in order; in each, the
    lowest valid lane of every key (its leader) looks for the key from h on, taking the first empty
    table slot (leaders of one input slot in lane order: one of the orders the CAS allows; which
    table slot a key gets may differ on the device, whether a probe wraps and how long a cluster is
    may not when every key of the tile is in the named set). Returns {"table": key -> table slot,
    "wrapped": keys whose probe went from slot 2047 to slot 0, "longest": most looks of one probe,
    "leaders": per input slot the number of leaders, "same_h": per input slot the most leaders that
    share one h, "counts": key -> (valid records, units): what the table's cells must hold}."""
    table, owner, wrapped, longest, leaders, same_h = {}, {}, set(), 0, [], []
    for s0 in range(0, tm.nin, SLOT):
        keys, seen = [], set()
        for q in range(s0, min(s0 + SLOT, tm.nin)):
            k = int(tm.key[q])
            if tm.fl[q] == 0 and k not in seen:
                seen.add(k)
                keys.append(k)
        leaders.append(len(keys))
        hs = hash_slot(keys).tolist() if keys else []
        same_h.append(max((hs.count(h) for h in set(hs)), default=0))
        for k, h in zip(keys, hs):
            looks = 1
            while owner.get(h, k) != k:
                if h == HT - 1:
                    wrapped.add(k)
                h = (h + 1) & (HT - 1)
                looks += 1
                assert looks <= HT
            owner[h] = k
            table[k] = h
            longest = max(longest, looks)
    return {"table": table, "wrapped": wrapped, "longest": longest, "leaders": leaders, "same_h": same_h,
            "counts": dict(tm.cells)}


# ------------------------------------------------------------------------------------------------
# tables
# ------------------------------------------------------------------------------------------------

@dataclass
class Table:
    name: str
    cfg: dict          # EngineConfig keywords (replication_factor 1: the transport run makes it 2)
    groups: list       # [[Case, ...], ...]
    notes: dict = field(default_factory=dict)

    def cases(self):
        return [c for g in self.groups for c in g]

    @property
    def P(self) -> int:
        return self.cfg["num_partitions"]


def cfg_for(P: int, depth: int, max_batch_records: int, segment_bytes: int, interval: int = 1024,
            max_batch_bytes: int = MIB) -> dict:
    return dict(num_partitions=P, replication_factor=1, segment_bytes=segment_bytes, index_interval=interval,
                max_consumers=2, max_batch_records=max_batch_records, pipeline_depth=depth,
                max_batch_bytes=max_batch_bytes)


def packed(name: str, pidx, lens, tag: int) -> Case:
    lens = np.asarray(lens, np.uint32)
    pay = _rng(1000 + tag).integers(0, 256, int(lens.sum(dtype=np.uint64)), dtype=np.uint8)
    return Case(name, Batch(np.asarray(pidx, np.int64).astype(np.uint32), lens, pay))


def small_lens(n: int, tag: int, hi: int = 200) -> np.ndarray:
    return _rng(tag).integers(0, hi + 1, n, dtype=np.uint32)


# ---- runs: partition runs laid out by sorted position, P = 8 ------------------------------------

RUN_TILES = {
    # name: the [start, end) of the tile's runs in sorted order, one partition each, ascending
    "pairs": [(0, 63), (63, 65), (65, 127), (127, 129), (129, 255), (255, 257), (257, 1024)],
    "slot-and-rest": [(0, 64), (64, 512), (512, 1024)],
    "head-at-511": [(0, 511), (511, 1024)],
    "one-partition": [(0, 1024)],
    "first-and-last": [(0, 1), (1, 1023), (1023, 1024)],
}
RUN_PARTS = {"pairs": [0, 1, 2, 3, 4, 5, 6], "slot-and-rest": [1, 3, 6], "head-at-511": [2, 5],
             "one-partition": [4], "first-and-last": [0, 3, 7]}
# the edges each tile is there for, per geometry (run_edges)
RUN_EDGES = {
    "pairs": {"single": {"starts_at_lane_63", "ends_at_lane_0", "crosses_slot_in_wave", "crosses_wave",
                         "two_whole_waves_without_head"},
              "transport": {"starts_at_lane_63", "ends_at_lane_0", "crosses_slot_in_wave", "crosses_wave",
                            "two_whole_waves_without_head"}},
    "slot-and-rest": {"single": {"crosses_wave", "head_only_in_first_slot_of_wave"},
                      "transport": {"crosses_wave", "two_whole_waves_without_head", "head_only_in_first_slot_of_wave"}},
    "head-at-511": {"single": {"starts_at_lane_63", "head_only_in_last_slot_of_wave", "two_whole_waves_without_head"},
                    "transport": {"starts_at_lane_63", "head_only_in_last_slot_of_wave", "two_whole_waves_without_head"}},
    "one-partition": {"single": {"whole_tile", "two_whole_waves_without_head"},
                      "transport": {"whole_tile", "two_whole_waves_without_head"}},
    "first-and-last": {"single": {"single_item_run", "starts_at_lane_63", "two_whole_waves_without_head"},
                       "transport": {"single_item_run", "starts_at_lane_63", "two_whole_waves_without_head"}},
}


def table_runs() -> Table:
    """Two batches of five full tiles in one launch group. The first gives every tile's records
    sorted by partition, so input order is sorted order and run k takes the positions RUN_TILES
    names; the second holds the same tiles, each shuffled by a fixed permutation (stage 1 ranks
    stably: the same runs at the same sorted positions, reached from scattered inputs). Record sizes
    vary from record to record (1 to 13 units)."""
    pidx = []
    for name, runs in RUN_TILES.items():
        tile = np.zeros(TILE_RECS, np.int64)
        for (a, b), p in zip(runs, RUN_PARTS[name]):
            tile[a:b] = p
        pidx.append(tile)
    srt = np.concatenate(pidx)
    n = srt.size
    shuf = np.concatenate([t[_rng(10 + k).permutation(TILE_RECS)] for k, t in enumerate(pidx)])
    group = [packed("sorted", srt, small_lens(n, 20, 192), 20), packed("shuffled", shuf, small_lens(n, 21, 192), 21)]
    return Table("runs", cfg_for(8, 2, n, MIB), [group], {"tiles": list(RUN_TILES)})


# ---- nin: batch sizes around the slot, wave and tile boundaries, P = 5 ---------------------------

NIN_SIZES = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2048, 2049)
NIN_MIXES = ((1024, 1), (2048, 1025), (1, 1024, 2048), (1024, 1, 2048, 1025), (1025, 2048, 1, 1024))


def nin_batch(n: int, tag: int, zero: bool) -> Case:
    """n records over partitions 1..4 with every seventh aimed at a partition that does not exist
    (key 0, like the junk lanes past n). zero: records of partition 0 as well, the last record of the
    batch among them, so key 0's run holds valid records, unknown ones and junk lanes; without it
    partition 0 must get no cell in any tile."""
    g = _rng(tag)
    pidx = g.integers(1, 5, n).astype(np.int64)
    pidx[3::7] = 5 + (np.arange(len(pidx[3::7])) % 2) * (UNKNOWN - 5)  # 5 and 2^32 - 1 in turn
    if zero:
        pidx[::5] = 0
        pidx[n - 1] = 0
    return packed(f"n{n}{'z' if zero else ''}", pidx, small_lens(n, tag), tag)


def table_nin() -> Table:
    groups = []
    for k, n in enumerate(NIN_SIZES):
        for zero in (False, True):
            groups.append([nin_batch(n, 100 + 2 * k + zero, zero)])
    for k, mix in enumerate(NIN_MIXES):
        groups.append([nin_batch(n, 200 + 10 * k + j, bool((k + j) % 2)) for j, n in enumerate(mix)])
    return Table("nin", cfg_for(5, 4, max(NIN_SIZES), MIB), groups)


# ---- keys: one table per key width -----------------------------------------------------------------

KEY_PS = (1, 2, 255, 256, 257, 1024, 65536)
KEY_WIDTHS = {1: (0, 0), 2: (1, 1), 255: (8, 1), 256: (8, 1), 257: (9, 2), 1024: (10, 2), 65536: (16, 2)}
EXTREMES_65536 = (0, 255, 256, 65279, 65280, 65535)  # low digit and high digit all zeros / all ones


def big_cfg() -> dict:
    """The P = 65536 engine: rings of 4 KiB (the smallest ring of 16 intervals of 256 B), one replica.
    Device memory on an MI355X by the driver's count: 454 MiB at creation and 18 MiB of staging with
    the first host batch, 472 MiB in all. Of it 256 MiB are rings (65536 x 4 KiB), 96 MiB index
    entries ((2 x depth + 2) = 6 entries of 16 B per interval of ring), 31 MiB ranking scratch (6 sets
    x 4 tiles x 65536 cells of 20 B), the rest per-partition words and allocation granules. With two
    replica slots (the transport run) an engine takes 710 MiB before its round buffers. A batch may
    hold at most 4096 - 256 stored bytes for one partition, so these tables keep the records of one
    partition in a batch few and short."""
    return cfg_for(65536, 2, 2048, 4096, interval=256)


def extremes(P: int) -> list:
    return sorted({0, P - 1, *(p for p in (1, 254, 255, 256, 257, P - 2) if 0 <= p < P),
                   *(EXTREMES_65536 if P == 65536 else ())})


def table_keys(P: int) -> Table:
    """P < 1024: a tile and a half of records over all partitions with the extremes present, then a
    short batch. P >= 1024: first a full tile of 1024 distinct partitions (every sorted item a head,
    every hash leader alone), the extremes among them, in a fixed shuffled order. Every table ends
    with a batch that repeats partitions, with records of unknown partitions at both ends."""
    g = _rng(300 + P % 9973)
    ext = extremes(P)
    cases = []
    if P >= 1024:
        rest = np.setdiff1d(np.arange(P), ext)
        distinct = np.concatenate([ext, g.choice(rest, TILE_RECS - len(ext), replace=False)])
        cases.append(packed("distinct", g.permutation(distinct), small_lens(TILE_RECS, 301), 301))
    n = 1500
    if P >= 1024:  # few partitions, so that they repeat inside a tile
        pidx = g.choice(np.concatenate([ext, g.choice(P, 40, replace=False)]), n).astype(np.int64)
    else:
        pidx = g.integers(0, P, n).astype(np.int64)
    pidx[10:10 + len(ext)] = ext
    pidx[TILE_RECS + 5:TILE_RECS + 5 + len(ext)] = ext[::-1]
    pidx[[0, 1, TILE_RECS - 1, TILE_RECS, n - 1]] = [P, UNKNOWN, P + 1, P, UNKNOWN]
    hi = 24 if P == 65536 else 200  # (4 KiB rings: some 35 records of a partition in the batch)
    cases.append(packed("repeats", pidx, small_lens(n, 302, hi), 302))
    cases.append(packed("short", pidx[:70][::-1].copy(), small_lens(70, 303, hi), 303))
    cfg = big_cfg() if P == 65536 else cfg_for(P, 2, 2048, 1 << 16 if P == 1024 else 1 << 18, interval=256)
    return Table(f"keys-P{P}", cfg, [cases[:-1], cases[-1:]], {"ext": ext})


# ---- hash: probe sequences that wrap and cluster, P = 65536 --------------------------------------

def table_hash() -> Table:
    """Partitions by their first table slot h (hash_slot). No h has more than 34 of the 65536
    partitions an engine may have, so 64 leaders of one h cannot exist: the crowded slots below hold
    64 leaders of 64 partitions that all start at one of two neighbouring h, 34 (the most there are)
    or 32 at the same one."""
    P = 65536
    h = hash_slot(np.arange(P))
    g = _rng(400)
    top, near = np.flatnonzero(h == HT - 1), np.flatnonzero(h >= HT - 4)
    count = np.bincount(h, minlength=HT)
    h0 = int(np.argmax(count[1:HT - 1])) + 1  # the fullest h away from the wrap
    crowd = np.concatenate([np.flatnonzero(h == h0), np.flatnonzero(h == h0 - 1)[:SLOT - int(count[h0])]])
    crowd_wrap = np.concatenate([np.flatnonzero(h == HT - 1)[:32], np.flatnonzero(h == HT - 2)[:32]])
    ordinary = g.choice(np.flatnonzero((h > 64) & (h < HT - 64)), 200, replace=False)
    lens = lambda n, tag: small_lens(n, tag, 40)
    mixed = np.concatenate([g.choice(top, 300), g.choice(near, 300), g.choice(ordinary, 360), crowd_wrap])
    mixed = mixed[g.permutation(mixed.size)]
    mixed[[7, 500]] = [UNKNOWN, P]
    groups = [
        [packed("h2047", g.choice(top, TILE_RECS), lens(TILE_RECS, 401), 401),
         packed("h2044+", g.choice(near, TILE_RECS), lens(TILE_RECS, 402), 402)],
        [packed("crowd", g.permutation(crowd), lens(SLOT, 403), 403),
         packed("crowd-wrap", g.permutation(crowd_wrap), lens(SLOT, 404), 404)],
        [packed("mixed", mixed, lens(mixed.size, 405), 405),
         packed("crowd-then-more", np.concatenate([g.permutation(crowd_wrap), g.choice(near, 130)]), lens(194, 406), 406)],
    ]
    return Table("hash", big_cfg(), groups, {"h0": h0, "most_per_h": int(count.max())})


# ---- flags: unknown partitions and bad explicit payload ranges inside runs, P = 16 ----------------

FLAG_P = 16
FLAG_N = TILE_RECS + 200  # a full tile and a partial one


def _explicit(name: str, pidx, lens, tag: int, bad=()) -> Case:
    """Explicit offsets with gaps of 0..15 bytes between the payloads; D = the end of the last one.
    bad: (record, kind): "end" puts the record's last byte at D (one past the end: o + L == D + 1),
    "start" its first byte past D + 1 (o > D). Such records have L > 0."""
    lens = np.asarray(lens, np.uint32).copy()
    g = _rng(2000 + tag)
    for k, _ in bad:
        lens[k] = max(int(lens[k]), 1)
    gaps = g.integers(0, 16, len(lens))
    poff = (np.cumsum(gaps + np.concatenate([[0], lens[:-1]]))).astype(np.uint64)
    D = int(poff[-1]) + int(lens[-1])
    for k, kind in bad:
        poff[k] = D - int(lens[k]) + 1 if kind == "end" else D + 2
    b = Batch(np.asarray(pidx, np.int64).astype(np.uint32), lens, g.integers(0, 256, D, dtype=np.uint8))
    return Case(name, b, poff, declared=D, invalid=bool(bad))


def table_flags() -> Table:
    """Partitions: 0 (key 0, with the unknown records and the junk lanes), 7 (every record of it in
    the rejected batches' first tile is out of range), 9 (absent), 11 (alone: one record a tile),
    the rest random. Large records (1025 to 3000 B) sit in the 64-record slots of the flagged ones."""
    g = _rng(500)
    n = FLAG_N
    others = np.array([p for p in range(FLAG_P) if p not in (7, 9, 11)])

    def base(tag):
        gg = _rng(tag)
        pidx = others[gg.integers(0, len(others), n)].astype(np.int64)
        pidx[gg.choice(np.arange(64, 960), 12, replace=False)] = 7
        pidx[[300, TILE_RECS + 100]] = 11
        return pidx, small_lens(n, tag + 1)

    big_at = [5, 40, 70, 1000, 1020, TILE_RECS + 3, n - 2]
    big_len = [1025, 3000, 1500, 2047, 1040, 2999, 1026]

    # A: accepted. Unknown partitions first and last in both tiles (first and last of key 0's run),
    # next to large records; tile 1 holds no record of partition 0 (key 0: one unknown record and junk)
    pa, la = base(510)
    pa[[0, TILE_RECS - 1, TILE_RECS, n - 1]] = [FLAG_P, UNKNOWN, FLAG_P + 1, FLAG_P]
    tail = pa[TILE_RECS + 1:n - 1]  # (a view)
    tail[tail == 0] = 1
    la[big_at] = big_len
    a = _explicit("A-unknown", pa, la, 511)
    # B: rejected whole. Out-of-range records: first and last input position of tile 0, the first and
    # the last record of partition 3 in it, the only record of partition 11, all of partition 7; in
    # tile 1 the last record; one large record out of range, one on an unknown partition
    pb, lb = base(520)
    pb[[0, TILE_RECS - 1]] = [2, 5]
    pb[2] = FLAG_P  # unknown and out of range at once
    pb[70] = UNKNOWN  # a large record of an unknown partition
    p3 = np.flatnonzero(pb[:TILE_RECS] == 3)
    bad = [(0, "end"), (TILE_RECS - 1, "start"), (2, "end"), (int(p3[0]), "start"), (int(p3[-1]), "end"), (300, "end"),
           *((int(k), "end" if j % 2 else "start") for j, k in enumerate(np.flatnonzero(pb[:TILE_RECS] == 7))),
           (n - 1, "end"), (40, "end")]
    lb[big_at] = big_len
    b = _explicit("B-out-of-range", pb, lb, 521, bad)
    # C: accepted, after the rejected batch in the same group
    pc, lc = base(530)
    lc[[1, 63, 64, 1023]] = [1025, 1026, 2000, 3000]
    c = _explicit("C-after", pc, lc, 531)
    # second group: a rejected batch whose one bad record is the last of a partial tile, then packed
    pd, ld = base(540)
    d = _explicit("D-last-record", pd[:TILE_RECS + 1], ld[:TILE_RECS + 1], 541, [(TILE_RECS, "start")])
    pe, le = base(550)
    pe[[0, 1, 2]] = [FLAG_P, FLAG_P, UNKNOWN]
    le[[0, 3, 1023]] = [2000, 1025, 1100]
    e = packed("E-packed", pe, le, 551)
    # a valid batch at the rule's edges: o + L == D, (o == D, L == 0), (o == D + 1, L == 0)
    pf, lf = base(560)
    f = _explicit("F-edges", pf[:130], lf[:130], 561)
    f.batch.lens[[3, 64]] = 0
    f.poff[[3, 64]] = [f.declared, f.declared + 1]
    f.poff[127] = f.declared - int(f.batch.lens[127])
    cfg = cfg_for(FLAG_P, 3, 2048, 1 << 18, interval=256)
    return Table("flags", cfg, [[a, b, c], [d, e, f]],
                 {"all_invalid": 7, "alone": 11, "absent": 9, "big_at": big_at})


TABLES = ("runs", "nin", *(f"keys-P{P}" for P in KEY_PS), "hash", "flags")
POSITIONAL = ("runs", "nin")  # the tables that also run with RMQ_S1_WGS=1 and RMQ_STEAL=1


def table(name: str) -> Table:
    if name.startswith("keys-P"):
        return table_keys(int(name[6:]))
    return {"runs": table_runs, "nin": table_nin, "hash": table_hash, "flags": table_flags}[name]()


def touched(t: Table) -> list:
    """The partitions a table's records name, and the first and last of the engine."""
    P = t.P
    s = {0, P - 1}
    for c in t.cases():
        s |= {int(p) for p in np.unique(c.batch.pidx) if p < P}
    return sorted(s)
