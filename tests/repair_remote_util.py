"""Host model of rmq_repair_remote (FORMAT.md §10, "Remote repair") in numpy, built on
tests/repair_util.py and shared by tests/test_repair_remote_model.py (CPU, on per-rank oracles) and
tests/test_gpu_repair_remote.py. Input is one snapshot per rank: per local partition its state (with
`commit`), live index entries and the ring bytes of every local slot, its placement key, its
replica ranks and its leader slot. The model runs pass 0 (repair_util's verdicts and local donors),
then plays the rounds: candidates, the commit rule, the donor's checks and walk on the donor's own
rings, the response (optionally with a byte flipped in flight), the requester's walk of the span
and the install. It returns per rank the rings, the counters and what the rank served. Every
expected value of the GPU tests comes from here and from bytes read back before the damage, never
from the call under test.

Requests are listed in task order (partition, slot, segment); the engine's lists are in no
particular order, so a scenario that flips a response byte keeps to one span per response."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import repair_util as R
from ripplemq_amd.tier import _scan

SERVED, UNKNOWN, OUTSIDE, BADWALK = 0, 1, 2, 3
MAX_REQS, PEER_BYTES = 1 << 16, 64 << 20


@dataclass
class RankSnap:
    rank: int
    parts: dict      # p -> (state, index entries, {local slot: ring bytes})
    key: dict        # p -> placement key
    ranks: dict      # p -> replica ranks by slot
    leader_slot: dict


@dataclass
class RankResult:
    rings: dict                      # p -> {slot: bytes} after the call
    rows: dict                       # p -> (repaired, bytes, fetched, bytes_fetched, unrepaired), partitions of the range
    served: tuple = (0, 0)
    statuses: list = field(default_factory=list)  # (round, donor, p, slot, segment, status) of every request sent


def snapshot(eng, cfg, view, rank) -> RankSnap:
    """One rank's snapshot of an engine or an oracle placed by `view`."""
    rf = cfg.replication_factor
    slots = lambda p: [s for s in range(rf) if int(view.ranks[p][s]) == rank]  # noqa: E731
    parts = R.snapshot(eng, cfg, slots=slots)
    n = len(view.gp)
    return RankSnap(rank, parts, {p: int(view.gp[p]) for p in range(n)},
                    {p: [int(x) for x in view.ranks[p]] for p in range(n)},
                    {p: int(view.leader_slot[p]) for p in range(n)})


def apply_flips(snap: RankSnap, flips) -> RankSnap:
    return RankSnap(snap.rank, R.apply_flips(snap.parts, flips), snap.key, snap.ranks, snap.leader_slot)


def candidates(snap: RankSnap, p: int) -> list:
    """Donor candidates of partition p: the leader's rank first, then the other slots' ranks by
    ascending slot, without this rank and without duplicates."""
    rk = snap.ranks[p]
    out = []
    for q in [rk[snap.leader_slot[p]]] + list(rk):
        if q != snap.rank and q not in out:
            out.append(q)
    return out


def span_ok(span, expect, eoff) -> bool:
    """The §10 walk of a span laid out linearly: eoff - expect records from `expect`, each checked,
    landing exactly on its end."""
    want = eoff - expect
    if want > span.size // 16:
        return False
    k, nb, _ = _scan(span, expect, want, True, False)
    return k == want and nb == span.size


def serve(donor: RankSnap, rings, I, key, pos, end, expect, eoff):
    """(status, span bytes or None) of one request on the donor, against the donor's current rings."""
    p = next((q for q, k in donor.key.items() if k == key), None)
    if p is None or p not in donor.parts or not donor.parts[p][2]:
        return UNKNOWN, None
    st = donor.parts[p][0]
    sp, ep, so, eo, S = (int(st[k]) for k in ("log_start_pos", "log_end_pos", "log_start_offset", "log_end_offset",
                                               "segment_bytes"))
    sane = ep >= sp and ep - sp <= S and (sp | ep) % 16 == 0 and eo >= so
    if not (sane and (pos | end) % 16 == 0 and sp <= pos < end <= ep and end - pos <= S and
            so <= expect <= eoff <= min(eo, int(st["commit"]))):
        return OUTSIDE, None
    for slot in sorted(rings[p]):
        if R.passes(rings[p][slot], (pos, end, expect, eoff)):
            return SERVED, R.seg_bytes(rings[p][slot], pos, end).copy()
    return BADWALK, None


def model(snaps, I, ranges=None, dry=False, corrupt=(), rounds=None, peer_bytes=PEER_BYTES):
    """[RankResult per rank] of a collective rmq_repair_remote over the snapshots. ranges: per rank
    the partitions of its [first, first + n) (None: all of them). corrupt: (src, dst, at) flips of
    the next response src sends to dst (rmq_fault_corrupt_repair). rounds: RF - 1 unless given.
    peer_bytes: RMQ_REPAIR_PEER_BYTES; a pair that would pass it is not asked for that round (the
    model takes the pairs in task order, the engine in no particular order: keep to scenarios in
    which the budget admits all of a destination's pairs or none)."""
    W = len(snaps)
    ranges = [sorted(s.parts) if ranges is None or ranges[r] is None else list(ranges[r]) for r, s in enumerate(snaps)]
    flips = {(s, d): at for s, d, at in corrupt}
    rings = [{p: {sl: a.copy() for sl, a in rs.items()} for p, (_, _, rs) in s.parts.items()} for s in snaps]
    counts, pending, fetched, served, statuses = [], [], [], [[0, 0] for _ in range(W)], [[] for _ in range(W)]
    # pass 0: rmq_repair on each rank's range
    for r, s in enumerate(snaps):
        sub = {p: s.parts[p] for p in ranges[r]}
        new, cnt = R.model(sub, I)
        pend = []
        for p in ranges[r]:
            st, ents, rs = s.parts[p]
            for si, seg in enumerate(R.segments(st, ents, I)):
                ok = {sl: R.passes(a, seg) for sl, a in rs.items()}
                if not any(ok.values()):
                    pend += [(p, sl, si, seg) for sl in sorted(rs)]
            if not dry:
                rings[r][p] = new[p]
        counts.append(cnt)
        pending.append(pend)
        fetched.append({p: [0, 0] for p in ranges[r]})
    rf = max(len(rk) for s in snaps for rk in s.ranks.values())
    for j in range(rf - 1 if rounds is None else rounds):
        # the requests of the round, per (requester, donor), in task order
        asks = {}
        for r, s in enumerate(snaps):
            nbytes = {}
            for item in pending[r]:
                p, sl, si, seg = item
                if seg is None or seg[0] >= seg[1] or seg[3] > int(s.parts[p][0]["commit"]):
                    continue  # no bounds, or an uncommitted tail: never fetched
                cand = candidates(s, p)
                if j >= len(cand):
                    continue
                d = cand[j]
                if nbytes.get(d, 0) + seg[1] - seg[0] > peer_bytes:
                    continue  # over the destination's budget: a later round or call
                lst = asks.setdefault((r, d), [])
                nbytes[d] = nbytes.get(d, 0) + seg[1] - seg[0]
                assert len(lst) < MAX_REQS, "the model does not play the pair limit"
                lst.append(item)
        if not asks:
            break
        # every donor serves from its rings as the round found them, then every requester installs
        answers = {}
        for (r, d), lst in asks.items():
            out = []
            for p, sl, si, seg in lst:
                status, span = serve(snaps[d], rings[d], I, snaps[r].key[p], *seg)
                statuses[r].append((j, d, p, sl, si, status))
                if status == SERVED:
                    served[d][0] += 1
                    served[d][1] += seg[1] - seg[0]
                out.append((status, None if dry else span))
            if (d, r) in flips:  # the next response d sends to r: one byte of its data section
                at = flips.pop((d, r))
                sizes = [0 if sp is None else sp.size for _, sp in out]
                total = sum(sizes)
                at = total + at if at < 0 else at
                if 0 <= at < total:
                    k = next(i for i in range(len(out)) if at < sum(sizes[:i + 1]))
                    out[k][1][at - sum(sizes[:k])] ^= 0x5A
            answers[(r, d)] = out
        for (r, d), lst in asks.items():
            for item, (status, span) in zip(lst, answers[(r, d)]):
                p, sl, si, (pos, end, expect, eoff) = item
                if status != SERVED:
                    continue
                if not dry:
                    if span.size != end - pos or not span_ok(span, expect, eoff):
                        continue  # nothing is written: the next candidate
                    ring = rings[r][p][sl]
                    ring[np.arange(pos, end) % ring.size] = span
                pending[r].remove(item)
                fetched[r][p][0] += 1
                fetched[r][p][1] += end - pos
    out = []
    for r in range(W):
        rows = {p: (counts[r][p][0], counts[r][p][1], fetched[r][p][0], fetched[r][p][1], counts[r][p][2] - fetched[r][p][0])
                for p in ranges[r]}
        out.append(RankResult(rings[r], rows, tuple(served[r]), statuses[r]))
    return out


# ---- the world both test files fill: world 3 (or 2), RF 3, 2 partitions per rank, 8 KiB rings, a
# sparse-index entry every 256 bytes; records of 0-120 bytes plus a few of 1.5-3 KB (over 64 pieces,
# several intervals long, so some segments are empty); BATCHES rounds, after which retention has
# moved every led log's start and one segment wraps the ring end.
PPR, SEG, INTERVAL, BATCHES = 2, 1 << 13, 256, 6


def base_cfg(rf=3, **kw):
    from ripplemq_amd.engine import EngineConfig

    d = dict(num_partitions=1, replication_factor=rf, segment_bytes=SEG, index_interval=INTERVAL, max_consumers=4,
             max_batch_records=256, max_batch_bytes=1 << 16, pipeline_depth=1)
    d.update(kw)
    return EngineConfig(**d)


def batch(rank: int, b: int):
    """One round's batch of a rank over the partitions it leads (local pidx [0, PPR))."""
    rng = np.random.default_rng(7000 + 100 * rank + b)
    pidx, lens = [], []
    for p in range(PPR):
        small = [int(x) for x in rng.integers(0, 121, 14)]
        small[int(rng.integers(0, 14))] = int(rng.integers(1536, 3073))
        small += [0, 16, 17, 120]
        pidx += [p] * len(small)
        lens += small
    order = rng.permutation(len(pidx))
    pidx, lens = np.array(pidx, np.uint32)[order], np.array(lens, np.uint32)[order]
    return pidx, lens, rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)


def local_of(snap: RankSnap, gp: int) -> int:
    return next(p for p, k in snap.key.items() if k == gp)


def slot_of(snap: RankSnap, p: int) -> int:
    return sorted(snap.parts[p][2])[0]


def records(snap: RankSnap, p: int, slot: int):
    """[(offset, logical position, payload length)] of a clean local slot's retained log."""
    import scrub_util as U

    st, _, rs = snap.parts[p]
    ring = rs[slot]
    win = ring[np.arange(st["log_start_pos"], st["log_end_pos"]) % ring.size]
    k, bad, recs, _ = U.walk_window(win, st)
    assert bad == U.NONE, (snap.rank, p, slot, bad)
    return recs


CLASSES = ("payload", "crc", "len_top", "wrapped")


def flip_of(snap: RankSnap, p: int, slot: int, what: str, below: int | None = None, above: int = 0):
    """(flip, segment index, segment) of a damage class on a local slot: one byte of a record whose
    offset lies in [above, below) (below: the commit unless given)."""
    st, ents, rs = snap.parts[p]
    S = rs[slot].size
    segs = R.segments(st, ents, INTERVAL)
    below = int(st["commit"]) if below is None else below
    recs = [x for x in records(snap, p, slot) if above <= x[0] < below]
    if what == "wrapped":  # a record of the segment that wraps the ring end
        si = next(i for i, s in enumerate(segs) if s[0] < s[1] and s[0] % S > (s[1] - 1) % S)
        rec = next(x for x in recs if segs[si][0] <= x[1] < segs[si][1] and x[2] > 0)
        delta, mask = 16 + rec[2] // 2, 0x5A
    else:
        inner = recs[len(recs) // 3:]
        if what == "payload":
            rec = next(x for x in inner if 40 <= x[2] <= 120)
            delta, mask = 16 + rec[2] // 2, 0x5A
        elif what == "big":
            rec = next(x for x in inner if x[2] > 1024)
            delta, mask = 16 + 1100, 0x5A
        elif what == "crc":
            rec = next(x for x in inner if x[2] > 0)
            delta, mask = 12, 0x5A
        elif what == "len_top":  # the claimed length exceeds the ring
            rec = next(x for x in inner if x[2] < 120)
            delta, mask = 11, 0x5A
        else:
            raise ValueError(what)
        si = R.seg_of(segs, rec[1])
    return (slot, p, (rec[1] + delta) % S, mask), si, segs[si]


def same_segment_flip(snap: RankSnap, p: int, slot: int, seg, mask=0x3C):
    """A crc byte of the first record that starts in segment `seg` (bounds as another rank found
    them: positions and offsets are equal on every replica) on this rank's slot."""
    rec = next(x for x in records(snap, p, slot) if seg[0] <= x[1] < seg[1])
    S = snap.parts[p][2][slot].size
    return (slot, p, (rec[1] + 12) % S, mask)
