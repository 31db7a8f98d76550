"""Host model of rmq_repair (FORMAT.md §10, "Repair") in numpy, shared by tests/test_repair_model.py
(CPU, on the oracle) and tests/test_gpu_repair.py. From the partition states, the live index
entries and the full ring bytes of every local slot it cuts the §10 segments, judges every (slot,
segment) pair with the host walk (tier._scan with the checks on, over that segment's bytes, plus
the containment rules), picks donors (the lowest passing local slot) and returns the rings and the
counters the call must leave. Every expected value of the GPU tests comes from here and from bytes
read back before the damage, never from rmq_repair. Also the damage scenarios both files run.
"""
from __future__ import annotations

import numpy as np

import scrub_util as U
from ripplemq_amd.tier import _scan


def snapshot(eng, cfg, parts=None, slots=None):
    """{p: (state, index entries lo..hi as an [k][2] array of (offset, pos), {slot: ring bytes})} of
    an engine or the oracle. slots(p): the local slots (default: all)."""
    I = cfg.index_interval
    out = {}
    for p in (range(cfg.num_partitions) if parts is None else parts):
        st = eng.state(p)
        lo, hi = (st["log_start_pos"] + I - 1) // I, st["log_end_pos"] // I
        ents = eng.read_index(p, lo, hi - lo + 1) if lo <= hi else np.zeros((0, 2), np.uint64)
        local = range(cfg.replication_factor) if slots is None else slots(p)
        out[p] = (st, np.array(ents, np.uint64), {r: np.array(eng.read_segment(r, p)) for r in local})
    return out


def segments(st, ents, I):
    """The §10 segments of a log: [(pos, end, expect, eoff) or None], None where the containment
    rules refuse the segment (it has no bounds) or the log is impossible."""
    sp, ep, so, eo, S = (int(st[k]) for k in ("log_start_pos", "log_end_pos", "log_start_offset", "log_end_offset",
                                               "segment_bytes"))
    if not (ep >= sp and ep - sp <= S and (sp | ep) % 16 == 0 and eo >= so):
        return [None]
    lo, hi = (sp + I - 1) // I, ep // I
    if lo > hi:
        return [(sp, ep, so, eo)]
    b = [(so, sp)] + [(int(o), int(x)) for o, x in ents] + [(eo, ep)]
    segs = []
    for s in range(hi - lo + 2):
        (expect, pos), (eoff, end) = b[s], b[s + 1]
        ok = sp <= pos <= end <= ep and (pos | end) % 16 == 0 and so <= expect <= eoff <= eo
        segs.append((pos, end, expect, eoff) if ok else None)
    return segs


def seg_bytes(ring, pos, end):
    S = ring.size
    return ring[(np.arange(pos, end) % S)] if end > pos else np.zeros(0, np.uint8)


def passes(ring, seg) -> bool:
    if seg is None:
        return False
    pos, end, expect, eoff = seg
    want = eoff - expect
    if want > (end - pos) // 16:  # (more records than 16-byte pieces: no walk can land)
        return False
    k, nb, _ = _scan(seg_bytes(ring, pos, end), expect, want, True, False)
    return k == want and nb == end - pos


def model(snap, I):
    """(rings {p: {slot: bytes}} after the repair, counts {p: (segments_repaired, bytes_repaired,
    segments_unrepaired)}) of a repair over the snapshot's partitions."""
    rings, counts = {}, {}
    for p, (st, ents, rs) in snap.items():
        new = {r: a.copy() for r, a in rs.items()}
        rep = nbytes = unrep = 0
        for seg in segments(st, ents, I):
            ok = {r: passes(a, seg) for r, a in rs.items()}
            donor = min((r for r in ok if ok[r]), default=None)
            for r in sorted(rs):
                if ok[r]:
                    continue
                if donor is None:
                    unrep += 1
                    continue
                pos, end = seg[0], seg[1]
                at = np.arange(pos, end) % rs[r].size
                new[r][at] = rs[donor][at]
                rep += 1
                nbytes += end - pos
        rings[p], counts[p] = new, (rep, nbytes, unrep)
    return rings, counts


def seg_of(segs, pos):
    """Index of the segment that holds logical position pos."""
    return next(i for i, s in enumerate(segs) if s is not None and s[0] <= pos < s[1])


def log_ok(ring, st) -> bool:
    """walk_window over a ring's retained window accepts the whole log."""
    S = ring.size
    win = ring[np.arange(st["log_start_pos"], st["log_end_pos"]) % S]
    return U.walk_window(win, st)[1] == U.NONE


# ---- the damage scenarios: lists of (slot, partition, ring offset, mask)
CLASSES1 = ("payload", "padding", "crc", "offset", "len_low", "len_top", "straddle", "first", "last")
CLASS_SLOT = 2


def class_flip(recs, S, what, p):
    from test_gpu_scrub import _pick  # the flip classes of the scrub's tests

    rec, delta, mask = _pick(recs, S, what)
    return rec, (CLASS_SLOT, p, (rec[1] + delta) % S, mask)


def class_partition(what):
    return 0 if what == "straddle" else 3


MULTI_P, OTHER_P = 4, 5


def multi_flips(recs4, recs5, segs4, S, which):
    """Several pairs in one call (partition MULTI_P; OTHER_P is damaged in the same call on slot 1).
    distinct: slots 0 and 2 in different segments. same: slots 0 and 1 in the same segment at
    different records. all3: the same segment on all three slots."""
    crc = lambda rec: (rec[1] + 12) % S  # noqa: E731 - a crc byte of the record
    other = (1, OTHER_P, crc(recs5[len(recs5) // 2]), 0x5A)
    if which == "distinct":
        a, b = recs4[3], recs4[-3]
        assert seg_of(segs4, a[1]) != seg_of(segs4, b[1])
        return [(0, MULTI_P, crc(a), 0x5A), (2, MULTI_P, crc(b), 0x5A), other]
    # two records that start in one segment
    a, b = next((x, y) for x, y in zip(recs4[2:], recs4[3:]) if seg_of(segs4, x[1]) == seg_of(segs4, y[1]))
    if which == "same":
        return [(0, MULTI_P, crc(a), 0x5A), (1, MULTI_P, crc(b), 0x5A), other]
    if which == "all3":
        return [(0, MULTI_P, crc(a), 0x5A), (1, MULTI_P, crc(b), 0x5A), (2, MULTI_P, crc(a), 0x3C), other]
    raise ValueError(which)


def apply_flips(snap, flips):
    """The flips on numpy copies of a snapshot's rings."""
    out = {p: (st, ents, {r: a.copy() for r, a in rs.items()}) for p, (st, ents, rs) in snap.items()}
    for slot, p, off, mask in flips:
        out[p][2][slot][off] ^= mask
    return out
