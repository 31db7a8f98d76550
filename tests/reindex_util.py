"""Host model of rmq_reindex (FORMAT.md §10, "Index rebuild") in numpy, on repair_util's snapshot /
segments / passes; shared by tests/test_reindex_model.py (CPU, on the oracle) and
tests/test_gpu_reindex.py. From a partition's state, its stored live entries and the ring bytes of
its local slots it rebuilds entries by the definition (E[m] = the first record start at logical
position >= m * I, the log end counting as one), in default mode (gaps of segments that pass on no
local slot, one walk per gap, resolved or not) and in ALL mode (one walk from the log start).
Every expected value of the GPU tests comes from here and from bytes read back before the damage,
never from rmq_reindex.
"""
from __future__ import annotations

import numpy as np

import repair_util as R
from ripplemq_amd.tier import _scan


def _sane(st) -> bool:
    sp, ep, so, eo, S = (int(st[k]) for k in ("log_start_pos", "log_end_pos", "log_start_offset", "log_end_offset",
                                               "segment_bytes"))
    return ep >= sp and ep - sp <= S and (sp | ep) % 16 == 0 and eo >= so


def live_range(st, I):
    """(lo, hi) of a sane log's live entries (lo > hi: none)."""
    return (int(st["log_start_pos"]) + I - 1) // I, int(st["log_end_pos"]) // I


def walk(rings, I, expect, pos, lim, m_first, m_last, m_check=None):
    """Walk the records from the record start (expect, pos) up to lim, accepting each on the lowest
    slot of `rings` on which it passes. A record start (o, x) gives {o, x} to every m in [m_first,
    m_last] (and m_check) not yet assigned with m * I <= x; the walk ends once m_check is assigned.
    Returns ({m: (o, x)}, the record start it stopped at, whether a record passed on no slot)."""
    out = {}
    top = m_last if m_check is None else m_check
    nxt = m_first

    def mark(o, x):
        nonlocal nxt
        while nxt <= top and nxt * I <= x:
            out[nxt] = (o, x)
            nxt += 1

    mark(expect, pos)
    while pos < lim and (m_check is None or m_check not in out):
        for i, r in enumerate(sorted(rings)):
            span = R.seg_bytes(rings[r], pos, lim)
            # every record the lowest slot accepts in a row; one record of any other slot
            k, _, at = _scan(span, expect, span.size // 16 if i == 0 else 1, True, True)
            if k:
                break
        else:
            return out, (expect, pos), True
        for j in range(1, k + 1):
            mark(expect + j, pos + int(at[j]))
            if m_check is not None and m_check in out:
                break
        expect, pos = expect + k, pos + int(at[k])
    return out, (expect, pos), False


def rebuild(st, rings, I):
    """The live entries of a clean log by the definition: an [hi - lo + 1][2] array, or None if the
    walk does not land on the log end."""
    lo, hi = live_range(st, I)
    so, sp, eo, ep = (int(st[k]) for k in ("log_start_offset", "log_start_pos", "log_end_offset", "log_end_pos"))
    out, end, dead = walk(rings, I, so, sp, ep, lo, hi)
    if dead or end != (eo, ep):
        return None
    return np.array([out[m] for m in range(lo, hi + 1)], np.uint64).reshape(-1, 2)


def gaps_of(st, ents, rings, I):
    """[(s_a, s_b)] of the maximal runs of segments that pass on no local slot."""
    segs = R.segments(st, ents, I)
    bad = [not any(R.passes(a, seg) for a in rings.values()) for seg in segs]
    out, s = [], 0
    while s < len(bad):
        if bad[s]:
            e = s
            while e + 1 < len(bad) and bad[e + 1]:
                e += 1
            out.append((s, e))
            s = e + 1
        else:
            s += 1
    return out, len(segs)


def model_part(st, ents, rings, I, all_mode=False):
    """(entries afterwards, entries_live, entries_rewritten, gaps_unresolved) of one partition."""
    ents = np.array(ents, np.uint64).reshape(-1, 2)
    if not rings:
        return ents, 0, 0, 0
    if not _sane(st):
        return ents, 0, 0, 1
    lo, hi = live_range(st, I)
    live = hi - lo + 1 if lo <= hi else 0
    so, sp, eo, ep = (int(st[k]) for k in ("log_start_offset", "log_start_pos", "log_end_offset", "log_end_pos"))
    if all_mode:
        gaps, nseg = [(0, live)], live + 1
    else:
        gaps, nseg = gaps_of(st, ents, rings, I)
    new, rewritten, unresolved = ents.copy(), 0, 0
    for a, b in gaps:
        last = b == nseg - 1
        expect, pos = (so, sp) if a == 0 else (int(ents[a - 1][0]), int(ents[a - 1][1]))
        stored = (eo, ep) if last else (int(ents[b][0]), int(ents[b][1]))
        lim = stored[1]
        if not (sp <= pos <= lim <= ep and (pos | lim) % 16 == 0 and so <= expect <= eo):
            unresolved += 1
            continue
        m_last = hi if last else lo + b - 1
        out, end, dead = walk(rings, I, expect, pos, lim, lo + a, m_last, None if last else lo + b)
        ok = not dead and (end == (eo, ep) if last else out.get(lo + b) == stored)
        if not ok:
            unresolved += 1
            continue
        for m in range(lo + a, m_last + 1):
            if tuple(int(x) for x in new[m - lo]) != out[m]:
                new[m - lo] = out[m]
                rewritten += 1
    return new, live, rewritten, unresolved


def model(snap, I, all_mode=False):
    """{p: (entries afterwards, entries_live, entries_rewritten, gaps_unresolved)} over a snapshot."""
    return {p: model_part(st, ents, rs, I, all_mode) for p, (st, ents, rs) in snap.items()}


def with_entries(snap, I, p, changes):
    """A snapshot copy with live entries of p XORed: changes = [(m, word, mask)]."""
    out = dict(snap)
    st, ents, rs = snap[p]
    ents = ents.copy()
    lo = live_range(st, I)[0]
    for m, word, mask in changes:
        ents[m - lo][word] ^= np.uint64(mask)
    out[p] = (st, ents, rs)
    return out
