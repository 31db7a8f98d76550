"""Device-memory append batches (RMQ_MEM_DEVICE) placed on purpose: the helper, the case tables and
the numpy model of what stage 3 does with a batch.

A device batch is read where the caller put it, and the on-device range check is all that stands
between its offsets and the kernels. DeviceBatch puts a payload at a chosen residue (and, for the
high-address cases, a chosen address) inside an allocation that holds every byte range the case
names, valid or invalid: a range check that failed would read the caller's own memory (0xFF filled),
never fault. classify() restates the thresholds of pipeline.hip's stage 3 so that
tests/test_append_edges_model.py can prove on the CPU that the tables hold the classes they are
named for; tests/test_gpu_append_device.py runs them against the oracle.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ripplemq_amd import _abi as A
from ripplemq_amd.engine import EngineConfig, EngineError
from ripplemq_amd.workload import Batch

# stage 3's thresholds (pipeline.hip / kernels.hpp)
TASK_RECS = 32      # kTaskRecs: records per stage-3 task (one wave, a lane pair per record)
TILE_RECS = 1024    # kTileRecs: records per stage-1 tile
IMG_PIECES = 7      # `m <= 7u` in stage3_finish / stage3_build: a wave whose stored records all have at
#                     most 7 payload pieces (112 B) stores through the LDS log image, else piece by piece
ROUND_PIECES = 8    # kPR: payload pieces per record per load round
BIG_PIECES = 64     # kBigPieces: records of more pieces (over 1024 B) go to the large-record waves
#                     (stage 1 decides the same for the group's list, `lenv > 16u * kBigPieces`)
SPAN_BLOCKS = 256   # 64 * kSpanPer: 16-byte blocks of a packed task's payload span staged through LDS

P, RF, SEG, INTERVAL, MAX_RECS = 8, 3, 1 << 18, 256, 4096
SHIFTS = (0, 4, 8, 12)  # rmq_append asks a device payload for 4-byte alignment only
LENS = (0, 1, 15, 16, 17, 111, 112, 113, 127, 128, 129, 143, 144, 145, 255, 256, 257, 1023, 1024, 1025, 1040, 2049)
ORDERS = ("sorted", "permuted")
OUT_UNWRITTEN = 0xA5A5A5A5A5A5A5A5  # the out-offset buffer before the append


def small_config(**kw) -> EngineConfig:
    base = dict(num_partitions=P, replication_factor=RF, segment_bytes=SEG, index_interval=INTERVAL,
                max_batch_records=MAX_RECS)
    base.update(kw)
    return EngineConfig(**base)


@dataclass
class Case:
    """One batch: `batch.payload` is the bytes at the payload address (gaps of explicit offsets
    included), `declared` the payload_bytes given to the engine (None: all of them)."""
    name: str
    batch: Batch
    poff: np.ndarray | None = None
    declared: int | None = None
    invalid: bool = False
    expect: set = field(default_factory=set)  # classes() this table is there for (at every shift)


# ---------------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------------
def record_starts(batch: Batch, poff=None) -> np.ndarray:
    if poff is not None:
        return np.asarray(poff, np.uint64).astype(np.int64)
    return batch.payload_offsets().astype(np.int64)


def classify(batch: Batch, shift: int = 0, poff=None) -> dict:
    """What stage 3 does with the batch when its payload sits at a 16-byte boundary + shift: per
    record m = ceil(L / 16) and sa = src & 15; per task of 32 records the store path (`image`: all
    m <= 7, `piecewise` otherwise, `big`: a record of m > 64), what its lane pairs do beside the
    large-record waves (`pair`), whether the payload span is staged (packed, at most 256 blocks from
    src0 & ~15 to the end of the last record) and the span's blocks."""
    lens = batch.lens.astype(np.int64)
    src = shift + record_starts(batch, poff)
    m = (lens + 15) // 16
    sa = src & 15
    tasks = []
    for i0 in range(0, batch.n, TASK_RECS):
        tm = m[i0:i0 + TASK_RECS]
        pair_m = tm[tm <= BIG_PIECES]  # big records are stored by the large-record waves
        pair = "image" if (pair_m <= IMG_PIECES).all() else "piecewise"
        path = "big" if (tm > BIG_PIECES).any() else pair
        i1 = min(i0 + TASK_RECS, batch.n) - 1
        blocks = int((src[i1] + lens[i1] - (src[i0] & ~15) + 15) >> 4)
        tasks.append({"i0": i0, "n": i1 - i0 + 1, "path": path, "pair": pair, "blocks": blocks,
                      "staged": poff is None and 0 < blocks <= SPAN_BLOCKS,
                      "long": int(((tm > IMG_PIECES) & (tm <= BIG_PIECES)).sum()), "bigs": int((tm > BIG_PIECES).sum())})
    return {"m": m, "sa": sa, "tasks": tasks}


def classes(batch: Batch, shift: int = 0, poff=None) -> set:
    """classify() as a set of names: `L<len>@<src & 15>` per record, `m<pieces>`, and per task
    `<path>`, `staged:<path>` / `unstaged:<path>`, `blocks<n>:staged|unstaged` (255..258), `empty_span`,
    `one_long` (31 image records and one stored piecewise), `one_big` (image records and one large
    record), `tail_task` (fewer than 32 records), `tiles<n>`."""
    c = classify(batch, shift, poff)
    out = {f"L{int(L)}@{int(s)}" for L, s in zip(batch.lens, c["sa"])}
    out |= {f"m{int(x)}" for x in c["m"]}
    out.add(f"tiles{-(-batch.n // TILE_RECS)}")
    for t in c["tasks"]:
        st = "staged" if t["staged"] else "unstaged"
        out |= {t["path"], f"{st}:{t['path']}"}
        if 255 <= t["blocks"] <= 258:
            out.add(f"blocks{t['blocks']}:{st}")
        if t["blocks"] == 0:
            out.add("empty_span")
        if t["n"] < TASK_RECS:
            out.add("tail_task")
        if t["long"] == 1 and t["bigs"] == 0:
            out.add("one_long")
        if t["bigs"] == 1 and t["long"] == 0:
            out.add("one_big")
    return out


# ---------------------------------------------------------------------------------------------
# case tables
# ---------------------------------------------------------------------------------------------
def _rng(tag: int) -> np.random.Generator:
    return np.random.Generator(np.random.Philox(key=[0x44455642, tag]))  # "DEVB"


def _crafted_tasks():
    """Three tasks appended to every length table (whole tasks, so they stay tasks): 31 records of
    at most 112 B and one of 113 B (the wave's __all turns the whole task piecewise), 31 such records
    and one of 1025 B (an image task beside a large-record wave), and an image task of 5 records."""
    short = [0, 1, 15, 16, 17, 111, 112, 96]
    a = [short[k % 8] for k in range(32)]
    b = list(a)
    a[17], b[9] = 113, 1025
    return a + b + [112, 96, 0, 17, 111]


def _targets(order: str, per_len: int):
    """(L, residue) for every L of LENS and every residue 0..15, per_len // 16 times; `sorted`: by L
    (a task of 32 holds one length), `permuted`: a fixed permutation (mixed tasks)."""
    t = [(L, r) for L in LENS for _ in range(per_len // 16) for r in range(16)]
    if order == "permuted":
        t = [t[k] for k in _rng(1).permutation(len(t))]
    return t + [(L, (5 * k) % 16) for k, L in enumerate(_crafted_tasks())]


_RESIDUES = {f"L{L}@{r}" for L in LENS for r in range(16)}
_PIECES = {"m7", "m8", "m9", "m64", "m65"}


def explicit_table(order: str) -> Case:
    """Explicit payload offsets: every length at every start residue, 32 records per length, gaps
    of up to 15 bytes between the payloads."""
    lens, offs, cur = [], [], 0
    for L, r in _targets(order, 32):
        o = cur + ((r - cur) % 16)
        lens.append(L)
        offs.append(o)
        cur = o + L
    n = len(lens)
    b = Batch((np.arange(n) % P).astype(np.uint32), np.array(lens, np.uint32),
              _rng(2).integers(0, 256, cur, dtype=np.uint8))
    expect = _RESIDUES | _PIECES | {"unstaged:image", "unstaged:piecewise", "unstaged:big", "one_long", "one_big",
                                    "tail_task"}
    return Case(f"explicit-{order}", b, np.array(offs, np.uint64), expect=expect)


def packed_table(order: str) -> Case:
    """Packed payloads: every length at every start residue, each steered there by a filler record
    of 0..15 bytes in front of it (a record like any other). A sorted table's tasks hold 16 fillers
    and 16 records of one length: staged image tasks up to 112 B, staged piecewise tasks up to 145 B,
    unstaged ones above, large records beside fillers from 1025 B."""
    lens, cur = [], 0
    for k, (L, r) in enumerate(_targets(order, 16)):
        if k < 16 * len(LENS):  # (the crafted tasks stay whole: no fillers)
            f = (r - cur) % 16
            lens.append(f)
            cur += f
        lens.append(L)
        cur += L
    n = len(lens)
    b = Batch((np.arange(n) % P).astype(np.uint32), np.array(lens, np.uint32),
              _rng(3).integers(0, 256, cur, dtype=np.uint8))
    expect = _RESIDUES | _PIECES | {"staged:image", "staged:piecewise", "unstaged:piecewise", "unstaged:big",
                                    "one_long", "one_big", "tail_task"}
    return Case(f"packed-{order}", b, expect=expect)


def length_tables() -> list[Case]:
    return [f(o) for f in (explicit_table, packed_table) for o in ORDERS]


def packed_case(name: str, lens, tag: int = 4, declared=None, invalid=False, expect=()) -> Case:
    lens = np.asarray(lens, np.uint32)
    n = len(lens)
    b = Batch((np.arange(n) % P).astype(np.uint32), lens, _rng(tag).integers(0, 256, int(lens.sum()), dtype=np.uint8))
    return Case(name, b, declared=declared, invalid=invalid, expect=set(expect))


TAIL_COUNTS = (1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049)


def span_cases() -> list[tuple[Case, int]]:
    """(case, shift): a task whose span is exactly 256 blocks (staged), 257 by a 4-byte shift and 257
    by one more byte (not staged), and an empty span."""
    return [(packed_case("span-32x128", [128] * 32, expect={"blocks256:staged"}), 0),
            (packed_case("span-32x128", [128] * 32, expect={"blocks257:unstaged"}), 4),
            (packed_case("span-4097", [128] * 31 + [129], expect={"blocks257:unstaged"}), 0),
            (packed_case("span-empty", [0] * 40, expect={"empty_span", "tail_task"}), 0)]


def tail_case(n: int) -> Case:
    """n records of 100 B: a task's tail (n % 32) and a tile's tail (n % 1024); declared is the exact
    payload size, so the last span ends at the last declared byte."""
    want = {f"tiles{-(-n // TILE_RECS)}"} | ({"tail_task"} if n % TASK_RECS else set())
    return packed_case(f"tail-{n}", [100] * n, tag=100 + n, expect=want)


def mixed40() -> Case:
    """The first 40 records of the permuted packed table as a batch of their own."""
    t = packed_table("permuted").batch
    lens = t.lens[:40]
    return Case("mixed40", Batch(t.pidx[:40].copy(), lens.copy(), t.payload[:int(lens.sum())].copy()))


RANGE_N = TILE_RECS + 6  # two tiles
# where the single offending record of an invalid explicit-offset batch goes
RANGE_PLACES = {"tile0": 5, "tile1": TILE_RECS + 3, "no_partition": 9}
RANGE_KINDS = ("end_plus_1", "start_plus_1")


def explicit_range_case(kind: str | None = None, place: str | None = None) -> Case:
    """1030 records of 20 B at offsets 24 i, payload_bytes D = 24 n. The valid batch holds the edges
    the rule allows: o + L == D, (o == D, L == 0) and (o == D + 1, L == 0: the rule is `L && ...`), in
    both tiles, and a record of an unknown partition. kind / place: one record replaced by one that
    breaks the rule by a single byte (o + L == D + 1, or o == D + 1 with L == 1)."""
    n = RANGE_N
    D = 24 * n
    lens = np.full(n, 20, np.uint32)
    poff = (24 * np.arange(n)).astype(np.uint64)
    pidx = (np.arange(n) % P).astype(np.uint32)
    pidx[11] = P + 1
    for k in (3, TILE_RECS + 1):
        poff[k] = D - 20          # o + L == D
    for k in (7, TILE_RECS + 2):
        poff[k], lens[k] = D, 0   # o == D, L == 0
    for k in (8, TILE_RECS + 4):
        poff[k], lens[k] = D + 1, 0
    name = "range-explicit-valid"
    if kind is not None:
        k = RANGE_PLACES[place]
        if place == "no_partition":
            pidx[k] = P + 3
        poff[k], lens[k] = (D - 19, 20) if kind == "end_plus_1" else (D + 1, 1)
        name = f"range-explicit-{kind}-{place}"
    b = Batch(pidx, lens, _rng(5).integers(0, 256, D, dtype=np.uint8))
    return Case(name, b, poff, declared=D, invalid=kind is not None)


def packed_range_case(n: int, over: int) -> Case:
    """n packed records of 20 B with payload_bytes = sum(len) - over: over 0 is the valid edge
    (sum == D), over 1 the invalid one (sum == D + 1)."""
    c = packed_case(f"range-packed-{n}-over{over}", [20] * n, tag=6)
    c.declared, c.invalid = 20 * n - over, over > 0
    return c


# ---------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------
class DeviceBatch:
    """A batch in device memory with its payload's first byte at alloc16 + shift, alloc16 a 16-byte
    boundary with 16 bytes of the allocation before it and `margin` bytes after the payload (every
    byte around the payload is 0xFF). at / region: alloc16 and the [lo, hi) of a caller's allocation
    instead of one of its own (only the bytes from alloc16 - 16 to the margin's end are written)."""

    def __init__(self, dev, batch: Batch, shift: int = 0, poff=None, declared: int | None = None,
                 margin: int = 64 << 10, at: int | None = None, region: tuple[int, int] | None = None):
        assert shift in SHIFTS
        self.dev, self.n, self.shift = dev, batch.n, shift
        self.pidx = np.ascontiguousarray(batch.pidx, np.uint32)
        self.lens = np.ascontiguousarray(batch.lens, np.uint32)
        self.poff = None if poff is None else np.ascontiguousarray(poff, np.uint64)
        pay = np.ascontiguousarray(batch.payload, np.uint8)
        self.declared = pay.size if declared is None else int(declared)
        self._own = []
        if at is None:
            size = 48 + pay.size + margin
            lo = self._alloc(size)
            hi, at = lo + size, (lo + 31) & ~15
        else:
            lo, hi = region
        assert at % 16 == 0 and lo <= at - 16
        self.lo, self.hi, self.payload_addr = lo, hi, at + shift
        # the invariant: every byte range the case names, valid or not, lies inside the allocation
        start = record_starts(batch, poff)
        ends = start + self.lens.astype(np.int64)
        named_end = max(int(ends.max(initial=0)), int(start.max(initial=0)), self.declared, pay.size)
        assert int(start.min(initial=0)) >= 0 and self.payload_addr + named_end + 16 <= hi, "a range leaves the allocation"
        assert self.payload_addr + pay.size + margin <= hi
        self.image = np.full(16 + shift + pay.size + margin, 0xFF, np.uint8)
        self.image[16 + shift:16 + shift + pay.size] = pay
        dev.h2d(at - 16, self.image)
        self.d_pidx, self.d_len = self._upload(self.pidx), self._upload(self.lens)
        self.d_poff = None if self.poff is None else self._upload(self.poff)
        self.d_out = self._upload(np.full(max(self.n, 1), OUT_UNWRITTEN, np.uint64))

    def _alloc(self, nbytes: int) -> int:
        p = self.dev.device_alloc(max(nbytes, 16))
        self._own.append(p)
        return p

    def _upload(self, a: np.ndarray) -> int:
        p = self._alloc(a.nbytes)
        if a.nbytes:
            self.dev.h2d(p, a)
        return p

    def submit(self) -> int:
        return self.dev.append_device(self.n, self.d_pidx, self.d_len, self.payload_addr, self.declared,
                                      self.d_out, self.d_poff)

    def read_out(self) -> np.ndarray:
        out = np.empty(self.n, np.uint64)
        if self.n:
            self.dev.d2h(out, self.d_out)
        return out

    def host_arrays(self):
        """(pidx, lens, the declared payload bytes, poff): what the oracle gets."""
        return self.pidx, self.lens, self.image[16 + self.shift:16 + self.shift + self.declared], self.poff

    def free(self) -> None:
        for p in self._own:
            self.dev.device_free(p)
        self._own = []


def device_case(dev, case: Case, shift: int = 0, **kw) -> DeviceBatch:
    return DeviceBatch(dev, case.batch, shift, case.poff, case.declared, **kw)


def check_result(ora, arrays, sd: dict, out: np.ndarray, invalid: bool, what: str = "") -> None:
    """The engine's stats and out offsets of one batch against the oracle given the same arrays.
    invalid: the oracle must refuse them with RMQ_EINVAL (its range_check is the rule), and the
    engine must have rejected the whole batch as the header documents."""
    pidx, lens, pay, poff = arrays
    n = len(pidx)
    if invalid:
        try:
            ora.append(pidx, lens, pay, poff)
        except EngineError as ex:
            assert ex.status == A.RMQ_EINVAL, (what, ex)
        else:
            raise AssertionError(f"{what}: the oracle accepted a batch the case calls invalid")
        want = dict.fromkeys(sd, 0)
        want.update(records=n, rejected_invalid=n)  # appended and every other rejection count: 0
        assert sd == want, f"{what}: stats of an invalid batch {sd}"
        assert (out == A.RMQ_OFFSET_NONE).all(), f"{what}: out offsets of an invalid batch {out[out != A.RMQ_OFFSET_NONE][:4]}"
        return
    oo, so = ora.append(pidx, lens, pay, poff)
    assert sd == so, f"{what}: append stats gpu={sd} cpu={so}"
    if not np.array_equal(out, oo):
        bad = np.flatnonzero(out != oo)
        raise AssertionError(f"{what}: out_offsets differ at {bad[:8]}: gpu={out[bad[:8]]} cpu={oo[bad[:8]]}")


def check_ticket(dev, ora, db: DeviceBatch, ticket: int, invalid: bool = False, what: str = "") -> dict:
    sd = dev.wait(ticket)
    check_result(ora, db.host_arrays(), sd, db.read_out(), invalid, what)
    return sd


def append_device_checked(dev, ora, db: DeviceBatch, invalid: bool = False, what: str = "") -> dict:
    """append_device, wait, out offsets back by d2h, the same arrays to the oracle: offsets and stats
    must agree, or (invalid) the whole batch is rejected_invalid on the device and RMQ_EINVAL there."""
    return check_ticket(dev, ora, db, db.submit(), invalid, what)


def append_pinned_checked(dev, ora, case: Case) -> dict:
    """The case through append_pinned_async (page-locked arrays, the same device check)."""
    b = case.batch
    n = b.n
    declared = b.payload.size if case.declared is None else case.declared
    ends = record_starts(b, case.poff) + b.lens.astype(np.int64)
    size = max(b.payload.size, declared, int(ends.max(initial=0))) + 16  # every named range inside the array
    pidx, lens, out = dev.host_empty(n, np.uint32), dev.host_empty(n, np.uint32), dev.host_empty(n, np.uint64)
    pay = dev.host_empty(size, np.uint8)
    pidx[:], lens[:], out[:], pay[:] = b.pidx, b.lens, OUT_UNWRITTEN, 0xFF
    pay[:b.payload.size] = b.payload
    poff = None
    if case.poff is not None:
        poff = dev.host_empty(n, np.uint64)
        poff[:] = case.poff
    sd = dev.wait(dev.append_pinned_async(pidx, lens, pay, out, payload_off=poff, payload_bytes=declared))
    check_result(ora, (b.pidx, b.lens, np.array(pay[:declared]), case.poff), sd, np.array(out), case.invalid, case.name)
    return sd  # (the page-locked arrays are freed with the engine)
