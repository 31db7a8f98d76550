"""Host model of rmq_restore (FORMAT.md §11) in numpy, shared by tests/test_restore_model.py (CPU, on
the oracle) and tests/test_gpu_restore.py, as repair_util.py is for rmq_repair. From a run's bytes,
its position table, the item, S_p, I and the local slots it gives the row the call must return and,
for a run that passes, the state fields, every slot's ring bytes and the live index entries the
call must leave. A record's CRC32C and padding verdict comes from the host walk (tier._scan with
the checks on, over that record's bytes) and the table rules are restated here; nothing comes from
rmq_restore. Also the scenarios both files run and the windows they take from an engine."""
from __future__ import annotations

import numpy as np

import scrub_util as U
from parity import ring_window
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import RESTORE_ITEM_DTYPE, EngineConfig
from ripplemq_amd.tier import _scan, record_positions

NONE = A.RMQ_OFFSET_NONE
CRC, CHAIN = A.RMQ_SCRUB_BAD_CRC, A.RMQ_SCRUB_BAD_CHAIN
STATE_FIELDS = ("log_start_offset", "log_start_pos", "log_end_offset", "log_end_pos", "commit", "high_watermark",
                "match", "segment_bytes")


def item(p, first_offset, first_pos, count, nbytes, buf_pos=0, table_start=0, commit=None, flags=0):
    it = np.zeros(1, RESTORE_ITEM_DTYPE)
    it[0] = (p, flags, first_offset, first_pos, count, nbytes, buf_pos, table_start,
             first_offset + count if commit is None else commit)
    return it


def _one(it):
    return it[0] if getattr(it, "shape", ()) else it


def judge(run, tab, it):
    """(bad_offset, bad_kind) of the lowest failing record under §11's device checks, or None."""
    it = _one(it)
    run = np.ascontiguousarray(run, np.uint8)
    n, nb, fo = int(it["count"]), int(it["bytes"]), int(it["first_offset"])
    for k in range(n):
        t0, t1 = int(tab[k]), int(tab[k + 1])
        if not (t0 % 16 == 0 and t1 % 16 == 0 and t0 < t1 <= nb and (k != 0 or t0 == 0) and (k + 1 != n or t1 == nb)):
            return fo + k, CHAIN
        off = int(run[t0:t0 + 8].view(np.uint64)[0])
        ln = int(run[t0 + 8:t0 + 12].view(np.uint32)[0])
        if off != fo + k or 16 + ((ln + 15) & ~15) != t1 - t0:
            return fo + k, CHAIN
        if _scan(run[t0:t1], fo + k, 1, True, False)[:2] != (1, t1 - t0):
            return fo + k, CRC
    return None


def host_refuses(run, tab, it) -> bool:
    """The host walk over the whole run plus the table rules refuse the input (the CPU assertion of
    the every-byte sweep: it does not go through judge's per-record slices)."""
    it = _one(it)
    n, nb, fo = int(it["count"]), int(it["bytes"]), int(it["first_offset"])
    k, got, pos = _scan(np.ascontiguousarray(run, np.uint8), fo, n, True, True)
    if k != n or got != nb:
        return True
    return not np.array_equal(np.asarray(tab[:n + 1], np.uint64), pos.astype(np.uint64))


def model(run, tab, it, S, I, slots, rf):
    """{"row": (status, records, bytes, bad_offset, bad_kind)} and, for a run that passes, "state",
    "rings" {slot: the S ring bytes of a ring that was all zero} and "index" (lo, entries [k][2])."""
    it = _one(it)
    run = np.ascontiguousarray(run, np.uint8)
    bad = judge(run, tab, it)
    if bad is not None:
        return {"row": (A.RMQ_ECORRUPT, 0, 0, bad[0], bad[1])}
    n, nb, fo, fp = int(it["count"]), int(it["bytes"]), int(it["first_offset"]), int(it["first_pos"])
    ring = np.zeros(S, np.uint8)
    ring[(fp + np.arange(nb)) % S] = run[:nb]
    lo, hi = (fp + I - 1) // I, (fp + nb) // I
    ents = {}
    if fp % I == 0:
        ents[fp // I] = (fo, fp)
    for k in range(n):
        pos, end = fp + int(tab[k]), fp + int(tab[k + 1])
        for m in range(pos // I + 1, end // I + 1):
            ents[m] = (fo + k + 1, end)
    assert sorted(ents) == list(range(lo, hi + 1)), (sorted(ents), lo, hi)
    leo = fo + n
    state = {"log_start_offset": fo, "log_start_pos": fp, "log_end_offset": leo, "log_end_pos": fp + nb,
             "commit": int(it["commit"]), "high_watermark": int(it["commit"]), "leader_commit": int(it["commit"]),
             "match": [leo if r in slots else 0 for r in range(rf)], "segment_bytes": S}
    index = np.array([ents[m] for m in range(lo, hi + 1)], np.uint64).reshape(-1, 2)
    return {"row": (A.RMQ_OK, n, nb, NONE, 0), "state": state, "rings": {r: ring for r in slots}, "index": (lo, index)}


def window(eng, cfg, p, slot=0):
    """Partition p's exact retained window of an engine or the oracle: (run bytes, table, item)."""
    st = eng.state(p)
    run = np.array(ring_window(eng, cfg, slot, p, st))
    n = st["log_end_offset"] - st["log_start_offset"]
    tab = (record_positions(run, n, st["log_start_offset"]) if n else np.zeros(1, np.int64)).astype(np.uint64)
    assert len(tab) == n + 1 and int(tab[-1]) == run.size
    return run, tab, item(p, st["log_start_offset"], st["log_start_pos"], n, run.size, commit=st["commit"])


def pack(windows, gap=48, order=None):
    """One call's (items, buf, rec_pos) from {p: window}: runs in `order` with `gap` bytes of 0xEE
    between them and a spare table word between the tables."""
    order = list(windows) if order is None else order
    items, bufs, tabs, at, words = [], [], [], gap, 1
    bufs.append(np.full(gap, 0xEE, np.uint8))
    tabs.append(np.full(1, 0xEEEE, np.uint64))
    for p in order:
        run, tab, it = windows[p]
        it = it.copy()
        it["buf_pos"], it["table_start"] = at, words
        items.append(it)
        bufs += [run, np.full(gap, 0xEE, np.uint8)]
        tabs += [tab, np.full(1, 0xEEEE, np.uint64)]
        at += run.size + gap
        words += len(tab) + 1
    return np.concatenate(items), np.concatenate(bufs), np.concatenate(tabs)


def assert_installed(eng, cfg, p, m, slots=None):
    """Engine state, every slot's window bytes and the live index entries equal the model's."""
    st = eng.state(p)
    for f in STATE_FIELDS:
        assert st[f] == m["state"][f], (p, f, st[f], m["state"][f])
    assert st["leader_commit"] == m["state"]["leader_commit"], (p, st)
    S = cfg.segment_bytes
    at = np.arange(st["log_start_pos"], st["log_end_pos"]) % S
    for r, ring in m["rings"].items():
        got = eng.read_segment(r, p)
        assert np.array_equal(got[at], ring[at]), (p, r)
    lo, ents = m["index"]
    if len(ents):
        assert np.array_equal(np.array(eng.read_index(p, lo, len(ents)), np.uint64), ents), (p, "index")


def pristine_snapshot(eng, cfg, p):
    """Everything a refused restore must leave: state, every ring byte of every slot, every index slot."""
    from parity import index_capacity

    st = eng.state(p)
    icap = index_capacity(cfg, st["segment_bytes"])
    return (st, [np.array(eng.read_segment(r, p)) for r in range(cfg.replication_factor)],
            np.array(eng.read_index(p, 0, icap)))


def assert_pristine(eng, cfg, p, before):
    st, rings, idx = pristine_snapshot(eng, cfg, p)
    assert st == before[0], (p, st, before[0])
    assert all(st[k] == 0 for k in ("log_start_offset", "log_start_pos", "log_end_offset", "log_end_pos", "commit",
                                    "high_watermark")), st
    for r, (a, b) in enumerate(zip(rings, before[1])):
        assert np.array_equal(a, b), (p, r, np.flatnonzero(a != b)[:8])
    assert np.array_equal(idx, before[2]), (p, "index slots")


# ---- scenarios
def cfg_main(**kw) -> EngineConfig:
    d = dict(num_partitions=8, replication_factor=3, segment_bytes=4096, index_interval=256, max_consumers=4,
             max_batch_records=256, max_batch_bytes=1 << 16)
    d.update(kw)
    return EngineConfig(**d)


def cfg_big() -> EngineConfig:
    return EngineConfig(num_partitions=8, replication_factor=3, segment_bytes=1 << 16, index_interval=256,
                        max_consumers=4, max_batch_records=256, max_batch_bytes=1 << 18)


def _batch(rng, pairs):
    pidx = np.array([p for p, _ in pairs], np.uint32)
    lens = np.array([n for _, n in pairs], np.uint32)
    return pidx, lens, rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)


def batches_main():
    """Partitions 0, 1: cycles of scrub_util.LENS1 (an empty payload, records over several intervals),
    six batches, so the rings wrap and retention runs; 2: twenty 256-byte records, a window of exactly
    S_p that starts on an interval; 3: one 16-byte record with an empty payload, alone; 4: two records
    of 3,840 bytes, the second alone in the window, on an interval; 5, 6, 7: 64, 65 and 129 records."""
    rng = np.random.default_rng(1100)
    out = []
    L = U.LENS1
    for b in range(6):
        pairs = [(p, L[(j + p + b) % len(L)]) for j in range(len(L)) for p in (0, 1)]
        if b < 2:
            pairs += [(2, 240)] * 10 + [(4, 3824)]
            pairs += [(7, (j + b) % 2) for j in range(65 - b)]
        if b == 0:
            pairs += [(3, 0)]
            pairs += [(5, 16 + j % 33) for j in range(64)] + [(6, j % 31) for j in range(65)]
        out.append(_batch(rng, pairs))
    return out


def more_main():
    """Further batches for every partition, enough for retention to run again everywhere."""
    rng = np.random.default_rng(1200)
    L = U.LENS1
    return [_batch(rng, [(p, L[(j + p + b) % len(L)]) for j in range(len(L)) for p in range(8)]) for b in range(3)]


def batches_big():
    """64 B to 16 KB records in 64 KiB rings (the whole-wave path), the last record of every partition
    large; partitions 0..3, three batches, so partition 0 wraps."""
    rng = np.random.default_rng(1300)
    out = []
    for b in range(3):
        pairs = []
        for p in range(4):
            lens = [int(x) for x in rng.integers(64, 16385, 2 + p)] + [64, 1009, 1024, 1025, 1040, 1041]
            lens.append(9000 + 1000 * p + b)  # the last record of the batch is large
            while sum(16 + ((x + 15) & ~15) for x in lens) > (1 << 16) - 256:
                lens.pop(0)
            pairs += [(p, x) for x in lens]
        out.append(_batch(rng, pairs))
    return out


def more_big():
    rng = np.random.default_rng(1400)
    return [_batch(rng, [(p, int(x)) for p in range(4) for x in rng.integers(64, 12000, 5)]) for _ in range(2)]


def fill(eng, batches):
    for b in batches:
        _, st = eng.append(*b)
        assert st["appended"] == len(b[0]), st


# ---- damage: flips of the run (the classes of repair_util.CLASSES1) and of the table
TABLE_CLASSES = ("table_word", "table_last", "table_zero")


def record_map(tab, run, it):
    """[(offset, logical position, payload length)] of a clean window (the record map _pick takes)."""
    fo, fp = int(it["first_offset"][0]), int(it["first_pos"][0])
    return [(fo + k, fp + int(tab[k]), int(run[int(tab[k]) + 8:int(tab[k]) + 12].view(np.uint32)[0]))
            for k in range(len(tab) - 1)]


def class_damage(run, tab, it, S, what):
    """(run, table) with the class's flip applied to copies."""
    run, tab = run.copy(), tab.copy()
    if what == "table_word":
        tab[len(tab) // 2] ^= np.uint64(0x40)
    elif what == "table_last":
        tab[-1] ^= np.uint64(0x10)
    elif what == "table_zero":
        tab[0] ^= np.uint64(0x10)
    else:
        from test_gpu_scrub import _pick  # the flip classes of the scrub's tests

        rec, delta, mask = _pick(record_map(tab, run, it), S, what)
        run[rec[1] - int(it["first_pos"][0]) + delta] ^= mask
    return run, tab


def consistent_padding(run, tab, k, crc32c):
    """(run, first padding byte, padding bytes) with record k's padding replaced by non-zero bytes
    that leave the CRC32C over its zero-padded pieces unchanged (scrub_util.crc_consistent_padding)."""
    run = run.copy()
    t0 = int(tab[k])
    ln = int(run[t0 + 8:t0 + 12].view(np.uint32)[0])
    pad = -ln % 16
    at = t0 + 16 + ln
    run[at:at + pad] = np.frombuffer(U.crc_consistent_padding(bytes(run[t0 + 16:at]), pad, crc32c), np.uint8)
    return run, at, pad
