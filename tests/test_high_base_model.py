"""The translation of the oracle to high coordinates (tests/high_base_util.py), pinned on the CPU
before any kernel is judged by it:

  * with every base (0, 0) the wrapper is the oracle;
  * at every base its state, window bytes and live index entries equal those of the restore model
    (restore_util.model: plain Python over arbitrary integers, no code shared with the wrapper) fed
    the oracle's window with first_offset, first_pos and the header offsets shifted here;
  * the comparators notice a shift truncated to 32 bits and a restamp that is off by one record;
  * the scenarios of tests/test_gpu_high_base.py do reach the edges they are there for (asserted on
    the oracle alone, with Python integers).
"""
import numpy as np
import pytest

import high_base_util as H
import restore_util as M
from parity import compare_state, run_ops
from ripplemq_amd import _abi as A

I = 256


class _DeviceSeat(H.Translated):
    """A wrapper in run_ops' device seat: append_async applies at once, wait hands the stats back."""

    def append_async(self, pidx, lens, payload, payload_off=None):
        out, st = self.append(pidx, lens, payload, payload_off)
        self.__dict__.setdefault("_stats", []).append(st)
        return len(self._stats) - 1, out

    def wait(self, ticket):
        return self._stats[ticket]


@pytest.fixture()
def make(oracle_mod):
    made = []

    def _make(cfg, bases=None, cls=H.Translated):
        ora = oracle_mod.OracleEngine(cfg)
        made.append(ora)
        if bases is None:
            return ora
        t = cls(ora, cfg, bases)
        H.rebase_oracle(t, bases)
        return t

    yield _make
    for o in made:
        o.close()


def _mixed_ops(bases):
    """scenario_ops and what else the wrapper translates: acks with remote slots, a ring move."""
    pp = np.arange(8, dtype=np.uint32)
    return H.scenario_ops(bases) + H.quorum_ops(bases) + [
        ("set_segments", pp[:3], np.full(3, 1 << 17, np.uint64)), ("append", H.scenario_batches(1, config_index=72)[0]),
        ("set_segments", pp[1:5], np.full(4, 1 << 14, np.uint64)),
        ("fetch", pp, np.zeros(8, np.uint32), np.full(8, 1024, np.uint32), 3000)]


def test_zero_base_wrapper_is_the_oracle(make):
    cfg = H.cfg_high()
    zero = {p: (0, 0) for p in range(8)}
    bare = make(cfg)
    H.rebase_oracle(bare, zero)
    run_ops(make(cfg, zero, _DeviceSeat), bare, cfg, _mixed_ops(zero), full_rings=True)


def _shifted_model(ora, cfg, p, dO, dP):
    """restore_util.model of the oracle's window of p moved to (dO, dP): the header offsets are
    shifted here, record by record of the window's own position table."""
    run, tab, it = M.window(ora, cfg, p)
    run, it = run.copy(), it.copy()
    for k in range(len(tab) - 1):
        t = int(tab[k])
        h = int.from_bytes(run[t:t + 8].tobytes(), "little") + dO
        run[t:t + 8] = np.frombuffer(h.to_bytes(8, "little"), np.uint8)
    it["first_offset"], it["first_pos"] = int(it["first_offset"][0]) + dO, int(it["first_pos"][0]) + dP
    it["commit"] = int(it["commit"][0]) + dO
    S = ora.state(p)["segment_bytes"]
    m = M.model(run, tab, it, S, cfg.index_interval, range(cfg.replication_factor), cfg.replication_factor)
    assert m["row"][0] == A.RMQ_OK, m["row"]
    return m


@pytest.mark.parametrize("interval", [256, 1024])
def test_wrapper_equals_the_restore_model_at_every_base(make, interval):
    cfg = H.cfg_high(index_interval=interval)
    bases = H.bases_for(interval)
    t = make(cfg, bases)
    checked = []

    def after(op, res):
        if op[0] not in ("append", "pipelined"):
            return
        for p in range(8):
            m = _shifted_model(t.ora, cfg, p, *bases[p])
            M.assert_installed(t, cfg, p, m)
            st = t.state(p)
            assert st["term_start"] == bases[p][0], st
            checked.append(p)

    H.apply_ops(t, H.scenario_ops(bases), after)
    assert len(checked) >= 8 * 8
    assert max(t.ora.state(p)["log_start_offset"] for p in range(8)) > 0, "retention must have run"


def test_fetch_rows_and_bytes_translate(make):
    """The wrapper's fetch is the oracle's with start_offset moved on the rows that name an offset
    of the log and with every served record's header restamped; nothing else changes."""
    cfg = H.cfg_high()
    bases = H.bases_for(I)
    t, o = make(cfg, bases), make(cfg, {p: (0, 0) for p in range(8)})
    seen = set()

    def after(op, res):
        if op[0] != "fetch":
            return
        rc, rows, buf, used = res
        ro, rows0, buf0, used0 = o.ora.fetch(op[1], op[2], op[3], op[4] if len(op) > 4 else None,
                                             commit=bool(op[5]) if len(op) > 5 else False)
        assert (rc, used) == (ro, used0)
        for f in ("out_pos", "count", "bytes", "status", "reserved"):
            assert np.array_equal(rows[f], rows0[f]), f
        for r, p in enumerate(int(x) for x in op[1]):
            assert int(rows["start_offset"][r]) == int(rows0["start_offset"][r]) + bases[p][0]
            seen.add(int(rows["status"][r]))
            lo, nb = int(rows["out_pos"][r]), int(rows["bytes"][r])
            if int(rows["status"][r]) == A.RMQ_OK and nb:
                off, pos = int(rows["start_offset"][r]), lo
                while pos < lo + nb:
                    assert int.from_bytes(buf[pos:pos + 8].tobytes(), "little") == off
                    assert np.array_equal(buf[pos + 8:pos + 16], buf0[pos + 8:pos + 16])
                    pos += 16 + ((int.from_bytes(buf[pos + 8:pos + 12].tobytes(), "little") + 15) & ~15)
                    off += 1
                assert off == int(rows["start_offset"][r]) + int(rows["count"][r])

    def run_both(op, res):
        if op[0] == "consumer_commit":  # the op names the rebased engine's offsets: the bare oracle's are less dO
            down = np.array([int(x) - bases[int(p)][0] for p, x in zip(op[1], op[3])], np.uint64)
            o.ora.commit_consumer_offset(op[1], op[2], down)
        elif op[0] == "append":
            o.ora.append(op[1].pidx, op[1].lens, op[1].payload)
        elif op[0] == "pipelined":
            for b in op[1]:
                o.ora.append(b.pidx, b.lens, b.payload)
        after(op, res)

    H.apply_ops(t, H.scenario_ops(bases), run_both)
    assert {A.RMQ_OK, A.RMQ_EOFFSET} <= seen, seen


# ---- sensitivity: a wrong translation must not pass the comparators (CPU only)
def test_comparators_notice_a_shift_truncated_to_32_bits(make):
    cfg = H.cfg_high()
    bases = H.bases_for(I)
    with pytest.raises(AssertionError):
        run_ops(make(cfg, bases), make(cfg, bases, H.Truncated32), cfg, H.scenario_ops(bases)[:1])
    # state alone: every base past 2^32 reads differently, the two that fit 32 bits do not
    a, b = make(cfg, bases), make(cfg, bases, H.Truncated32)
    diff = [p for p in range(8) if a.state(p) != b.state(p)]
    assert diff == [2, 4, 5, 7], diff


def test_comparators_notice_a_restamp_off_by_one_record(make):
    cfg = H.cfg_high()
    bases = H.bases_for(I)
    ops = H.scenario_ops(bases)
    with pytest.raises(AssertionError, match="ring p=0"):
        run_ops(make(cfg, bases), make(cfg, bases, H.StampOffByOne), cfg, ops[:1])
    with pytest.raises(AssertionError, match="fetched bytes differ"):
        run_ops(make(cfg, bases), make(cfg, bases, H.StampOffByOne), cfg, ops[:3], check=False)
    with pytest.raises(AssertionError):
        run_ops(make(cfg, bases), make(cfg, bases, H.OffsetsOffByOne), cfg, ops[:1], check=False)
    a, b = make(cfg, bases), make(cfg, bases, H.StampOffByOne)
    H.apply_ops(a, ops[:1])
    H.apply_ops(b, ops[:1])
    with pytest.raises(AssertionError, match="ring"):
        compare_state(a, b, cfg)


# ---- preconditions of the GPU scenarios, on the oracle alone
@pytest.mark.parametrize("group,I", [(1, 256), (2, 256), (3, 256), (2, 1024)])
def test_scenario_reaches_its_edges(make, group, I):
    cfg = H.cfg_high(pipeline_depth=group, index_interval=I)
    bases = H.bases_for(I)
    S = cfg.segment_bytes
    ora = make(cfg)
    for p in range(8):
        ora.become_leader(p, 2)
    both, retained_after, slice_over, interval_over, wrapped = set(), set(), set(), set(), set()
    ops = H.scenario_ops(bases, group)

    def down(op):  # the ops name the rebased engine's offsets: the bare oracle's are those less dO
        if op[0] != "consumer_commit":
            return op
        return (op[0], op[1], op[2], np.array([int(x) - bases[int(p)][0] for p, x in zip(op[1], op[3])], np.uint64))

    def after(op, res):
        for p, B in H.CROSSING.items():
            dO, dP = bases[p]
            st = ora.state(p)
            lo_p, hi_p = st["log_start_pos"] + dP, st["log_end_pos"] + dP
            lo_o, hi_o = st["log_start_offset"] + dO, st["log_end_offset"] + dO
            if op[0] in ("append", "pipelined"):  # a checked step: compare_state runs after it
                if lo_p < B <= hi_p and lo_o < B <= hi_o:
                    both.add(p)
                    if lo_p % S > hi_p % S or hi_p % S == 0:
                        wrapped.add(p)
                    m_lo, m_hi = -(-st["log_start_pos"] // I), st["log_end_pos"] // I
                    e = ora.read_index(p, m_lo, m_hi - m_lo + 1)
                    offs = [int(x) + dO for x in e[:, 0]]
                    if any(a < B < b for a, b in zip(offs, offs[1:])):
                        interval_over.add(p)
                if lo_o > B and lo_p > B and st["log_start_offset"] > 0:
                    retained_after.add(p)
            if op[0] == "fetch":
                rows = res[1]
                for r in np.flatnonzero((np.asarray(op[1]) == p) & (rows["status"] == A.RMQ_OK) & (rows["count"] > 0)):
                    a = int(rows["start_offset"][r])
                    b = a + int(rows["count"][r])
                    pa, pb = ora.record_pos(p, a), ora.record_pos(p, b)
                    if a + dO < B < b + dO and pa + dP < B < pb + dP:
                        slice_over.add(p)

    H.apply_ops(ora, [down(op) for op in ops], after)
    want = set(H.CROSSING)
    assert both == want, ("log straddles the boundary in offsets and positions at a checked step", both)
    assert wrapped == want, ("a window that straddles it wraps the ring end", wrapped)
    assert interval_over == want, ("an index interval's offsets straddle it", interval_over)
    assert slice_over == want, ("a fetched slice straddles it", slice_over)
    assert retained_after == want, ("retention runs after the crossing", retained_after)
    # every partition wraps its ring several times and stays clear of 2^59
    for p in range(8):
        st = ora.state(p)
        assert st["log_end_pos"] > 2 * S and st["log_start_offset"] > 0, (p, st)
        assert st["log_end_offset"] + bases[p][0] < 2 ** 59 and st["log_end_pos"] + bases[p][1] < 2 ** 59


@pytest.mark.parametrize("I", [256, 1024])
def test_first_batch_crosses_inside_a_record(make, I):
    """The byte that reaches 2^32 (2^31) lies inside a record, and the record of that offset is not
    the one of that byte: offsets and positions cross at different records."""
    cfg = H.cfg_high()
    bases = H.bases_for(I)
    ora = make(cfg)
    b = H.first_batch()
    ora.append(b.pidx, b.lens, b.payload)
    for p, B in H.CROSSING.items():
        dO, dP = bases[p]
        recs = H.window_records(ora, cfg, p)
        over = [o for o, pos, ln in recs if pos + dP < B < pos + dP + 16 + ((ln + 15) & ~15)]
        assert len(over) == 1 and over[0] + dO != B, (p, over)
        assert any(o + dO == B for o, _, _ in recs)


def test_world_steps_reach_their_edges(oracle_mod):
    """The replication script on the oracles alone: every lead is granted, the first fetch is served
    and the later one is RMQ_EOFFSET, rank 1 misses a round of rank 0 and is caught up (entries sent
    again, every follower at its leader's log end), every ring wraps, and the translated coordinates
    pass 2^32 and 2^31 on the partitions that cross and stay below 2^59."""
    from world_script import run_oracle

    views, cfgs, bases = H.world_setup()
    zero = [{p: (0, 0) for p in b} for b in bases]
    oras = [oracle_mod.OracleEngine(c) for c in cfgs]
    try:
        for r in range(H.WORLD):
            H.rebase_oracle(oras[r], bases[r])
        steps = H.world_steps(views, zero)
        out = run_oracle(oras, views, steps)
        assert all(s == A.RMQ_OK for r in range(H.WORLD) for s in out[0][r])
        kf = [k for k, s in enumerate(steps) if s[0] == "fetch"]
        assert all((out[kf[0]][r][1]["count"] == 20).all() for r in range(H.WORLD))
        assert all((out[kf[1]][r][1]["status"] == A.RMQ_EOFFSET).all() for r in range(H.WORLD))
        assert int(oras[0].counters()[4]) > 0, "catch-up entries sent by rank 0"
        ends = {}
        for r in range(H.WORLD):
            for p, g in enumerate(views[r].gp):
                st = oras[r].state(p)
                ends.setdefault(int(g), set()).add((st["log_start_offset"], st["log_end_offset"], st["log_end_pos"], st["commit"]))
                assert st["log_start_offset"] > 0 and st["log_end_pos"] > cfgs[r].segment_bytes
                dO, dP = bases[r][p]
                assert st["log_end_offset"] + dO < 2 ** 59 and st["log_end_pos"] + dP < 2 ** 59
                B = {1: 2 ** 32, 3: 2 ** 31}.get(int(g))  # the retained log has left the boundary behind
                assert B is None or (st["log_start_offset"] + dO > B and st["log_start_pos"] + dP > B)
        assert all(len(v) == 1 for v in ends.values()), ends  # every replica of a partition agrees
        assert all(sorted(int(g) for g in v.gp) == list(range(6)) for v in views)  # one partition per base
    finally:
        for o in oras:
            o.close()
