"""The scenarios of tests/test_gpu_ingest_sweep.py on the CPU oracle alone: each is what it claims
(the lengths, the flipped fields, the copy phases and the task edges are there), and every flip is
refused by the oracle in a way a follower that wrongly accepted it could not match, so the GPU tests
cannot pass vacuously."""
import hashlib

import numpy as np
import pytest

import ingest_util as X
import scrub_util as U

SCENARIOS = {"A": X.scenario_a, "B-places": X.scenario_b_places, "B2": X.scenario_b2, "B3": X.scenario_b3,
             "C": X.scenario_c, "D": X.scenario_d}
SCENARIOS.update({"B-" + f: (lambda f=f: X.scenario_b(f)) for f in X.FIELDS})
FLIPPED = [n for n in SCENARIOS if n.startswith("B")]


@pytest.fixture(scope="module")
def runs(oracle_mod):
    cache = {}

    def get(name, faults=True):
        if (name, faults) not in cache:
            sc = SCENARIOS[name]()
            cache[(name, faults)] = (sc, X.run_oracle(oracle_mod, sc, faults))
        return cache[(name, faults)]
    return get


def regions_of(run):
    for k, rnd in enumerate(run.clean):
        for s, row in enumerate(rnd):
            for d, reg in enumerate(row):
                if reg is not None and reg.size:
                    yield k, s, d, reg


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_region_map_reads_every_region(runs, name):
    sc, run = runs(name)
    seen = 0
    for k, s, d, reg in regions_of(run):
        m = X.region_map(reg)
        X.check_map(m)  # the records tile the data section, the table agrees, data_off / rows_off by §9
        assert (m["hdr"]["src"], m["hdr"]["n"], m["hdr"]["round"]) == (s, len(sc.pair_list(s, d)), k)
        seen += 1
    assert seen == sc.rounds * sc.world * (sc.world - 1)


def test_lengths_of_scenario_a(runs):
    sc, run = runs("A")
    assert len(X.LENS_I) == len(U.LENS3) + 6 and {63, 64, 65, 79, 80, 81} <= set(X.LENS_I) >= set(U.LENS3)
    assert set(X.B_LENS) <= set(X.LENS_I)
    last_pieces = set()
    for k, s, d, reg in regions_of(run):
        m = X.region_map(reg)
        for e in range(X.PARTS_I):  # every entry of every round carries every length once
            assert sorted(r["len"] for r in m["recs"] if r["entry"] == e) == sorted(X.LENS_I), (k, s, d, e)
        last_pieces.add((m["recs"][-1]["len"] + 15) // 16)
    assert 1 in last_pieces  # (the one count up to five that scenario D's cycle cannot end a region with)
    for r in range(sc.world):
        st = run.digests[-1][r]["states"]
        assert (st["log_start_offset"] > 0).all() and (st["log_end_pos"] > sc.cfg["segment_bytes"]).all(), r
    assert all(c[1] == c[2] == c[4] == c[5] == 0 for c in run.counters[-1])


def test_flip_list_of_scenario_b(runs):
    want = {(ln, f) for f in X.FIELDS for ln in X.b_lengths(f)}
    # 14 lengths with the four header fields, 13 with payload, 7 with padding
    assert len(want) == 14 * 4 + 13 * 2 + 7 * 2 and {ln for ln, _ in want} == set(X.B_LENS)
    got = set()
    for f in X.FIELDS:
        sc, run = runs("B-" + f)
        for k in range(sc.rounds - 1):
            (s, d, at), = run.flips[k]
            m = X.region_map(run.clean[k][s][d])
            rec, flds = X.field_at(m, at)
            assert (s, d) == (0, 1) and rec["entry"] == k % X.PARTS_I and f in flds, (f, k, rec, flds)
            got.add((rec["len"], f))
            if k:  # the entry refused the round before is a catch-up entry of this very region
                assert m["dir"][(k - 1) % X.PARTS_I]["count"] == 2 * X.NREC_I and m["rows"], (f, k)
        assert not run.flips[-1]
    assert got == want, (want - got, got - want)


def test_flip_list_of_the_places(runs):
    sc, run = runs("B-places")
    at = {}
    for k, name in enumerate(X.PLACES):
        (s, d, a), = run.flips[k]
        m = X.region_map(run.clean[k][s][d])
        at[name] = (m, *X.field_at(m, a))
    assert at["tab63"][1]["t"] == 63 and at["tab64"][1]["t"] == 64
    assert at["first_rec"][1]["k"] == 0 and at["first_rec"][1]["entry"] == 1
    m, rec, _ = at["last_rec"]
    assert rec["k"] == m["dir"][rec["entry"]]["count"] - 1
    m, rec, _ = at["gap"]  # entry 2, refused the round before: 95 records re-read from the leader's ring first
    assert m["dir"][2]["count"] == 2 * X.NREC_I and rec["entry"] == 2 and rec["k"] < X.NREC_I and rec["len"] > 1024
    assert at["big"][1]["len"] == 4097
    m, rec, flds = at["row_entry"]
    assert rec is None and flds == ["row_entry"] and [w["entry"] for w in m["rows"]] == [3]


@pytest.mark.parametrize("name", sorted(FLIPPED))
def test_every_flip_is_refused_and_seen(runs, name):
    sc, run = runs(name)
    _, clean = runs(name, faults=False)
    views = sc.views()
    zero_ring = hashlib.blake2b(bytes(sc.cfg["segment_bytes"]), digest_size=16).hexdigest()
    flips = 0
    for k in range(sc.rounds):
        want = {}
        for s, d, at in run.flips[k]:
            m = X.region_map(run.clean[k][s][d])
            want[(s, d)] = X.expected_refused(sc, m, s, d, at)
            flips += 1
        # exactly the expected entries are refused, and no entry of any other pair
        assert {sd: e for sd, e in run.refused[k].items() if e} == want, (name, k, run.refused[k], want)
        before = run.counters[k - 1] if k else [(0,) * 6] * sc.world
        for r in range(sc.world):
            now = run.counters[k][r]
            hit = [(s, d) for (s, d) in want if d == r]
            structural = [sd for sd in hit if len(want[sd]) == len(sc.pair_list(*sd))]
            # a record flip is one CRC refusal (the partition's other slot is refused with it, not
            # counted again); a structural fault counts every entry of the pair; never a log refusal
            n_crc = sum(len(want[sd]) if sd in structural else 1 for sd in hit)
            assert (now[1] - before[r][1], now[2] - before[r][2], now[5]) == (n_crc, 0, 0), (name, k, r, now, before[r])
            # every entry refused the round before is sent again as a catch-up entry
            resent = sum(len(e) for (s, d), e in (run.refused[k - 1].items() if k else ()) if s == r)
            assert now[4] - before[r][4] == resent, (name, k, r, now, before[r], resent)
        for (s, d), entries in want.items():
            pl = sc.pair_list(s, d)
            for e in entries:
                gp, slot = pl[e]
                p = int(np.flatnonzero(views[d].gp == gp)[0])
                st1 = run.digests[k][d]["states"][p]
                leo0 = int(run.digests[k - 1][d]["states"][p]["log_end_offset"]) if k else 0
                ring0 = run.digests[k - 1][d]["rings"][(p, slot)] if k else zero_ring
                assert int(st1["log_end_offset"]) == leo0, (name, k, d, p)
                assert run.digests[k][d]["rings"][(p, slot)] == ring0, (name, k, d, p, slot)
            # a follower that accepted the flipped region would hold the clean run's state and rings:
            # the digests tell the two apart
            diff = X.digest_diff(run.digests[k][d], clean.digests[k][d])
            assert any(w == "state" for w, _, _ in diff) and any(w == "ring" for w, _, _ in diff), (name, k, diff)
    assert flips == sum(len(v) for v in sc.plans.values()) > 0
    for r in range(sc.world):  # every follower caught up, and holds what a clean run holds
        st = run.digests[-1][r]["states"]
        for p in range(views[r].led):
            assert [int(x) for x in st[p]["match"][:sc.rf]] == [int(st[p]["log_end_offset"])] * sc.rf, (name, r, p)
        assert np.array_equal(st["log_end_offset"], clean.digests[-1][r]["states"]["log_end_offset"])
        assert run.digests[-1][r]["rings"] == clean.digests[-1][r]["rings"], (name, r)
    # the GPU tests' comparison itself: engines that behaved as in the clean run are told from this
    # run by the regions alone, by the counters alone and by the digests alone
    for part in ("regions", "counters", "digests"):
        other = X.Run(**{f: getattr(clean if f == part else run, f) for f in ("regions", "counters", "digests")})
        with pytest.raises(AssertionError, match=name + " round"):
            X.compare_runs(sc, other, run)
    X.compare_runs(sc, run, run)


def test_two_slots_and_two_sources(runs):
    sc, run = runs("B2")
    assert [sorted(v for v in rr.values() if v) for rr in run.refused] == [[[0, 1]], [[2, 3]], []]
    assert [c[1][1] for c in run.counters] == [1, 2, 2] and [c[0][4] for c in run.counters] == [0, 2, 4]
    assert len(sc.pair_list(0, 1)) == 2 * X.PARTS_I  # 760 records a region: 12 verify tasks, over one workgroup's 8 waves
    sc, run = runs("B3")
    assert [{sd: v for sd, v in rr.items() if v} for rr in run.refused] == [{}, {(0, 2): [0], (1, 2): [2]}, {}]
    m0, m1 = (X.region_map(run.clean[1][s][2]) for s in (0, 1))
    lens = [X.field_at(m, at)[0]["len"] for m, (_, _, at) in zip((m0, m1), sorted(run.flips[1]))]
    assert lens == [17, 4097]
    assert run.counters[1][2][1] == 2 and run.counters[2][0][4] == run.counters[2][1][4] == 1


def test_copy_edges_of_scenario_c(runs):
    sc, run = runs("C")
    S = sc.cfg["segment_bytes"]
    pairs, wrap_in_chunk = set(), 0
    for k, s, d, reg in regions_of(run):
        m = X.region_map(reg)
        if k == 0:
            assert [dd["bytes16"] for dd in m["dir"]] == list(range(X.C_PARTS))  # log ends at 16 p: phase p
            continue
        for e, dd in enumerate(m["dir"]):
            pos = int(run.digests[k - 1][s]["states"][e]["log_end_pos"])  # where the follower's copy starts
            assert 16 * dd["bytes16"] == X.C_SIZES[k - 1] and dd["first"] == int(run.digests[k - 1][s]["states"][e]["log_end_offset"])
            pairs.add(((pos >> 4) & 7, 16 * dd["bytes16"]))
            for c in range(0, 16 * dd["bytes16"], 16384):  # the copy's 16 KiB chunks
                a, b = pos + c, pos + min(c + 16384, 16 * dd["bytes16"])
                wrap_in_chunk += a // S != (b - 1) // S
    assert pairs == {(ph, sz) for ph in range(8) for sz in X.C_SIZES}
    assert wrap_in_chunk >= 8
    for r in range(sc.world):
        st = run.digests[-1][r]["states"]
        assert (st["log_end_pos"] > S).all() and (st["log_start_offset"] > 0).all()
    # the rings wrap from the fourth round on
    first = min(k for k in range(sc.rounds) if (run.digests[k][0]["states"]["log_end_pos"] > S).any())
    assert first == 4, first


def test_task_edges_of_scenario_d(runs):
    sc, run = runs("D")
    big_at, last_pieces = set(), set()
    for k, s, d, reg in regions_of(run):
        m = X.region_map(reg)
        assert m["hdr"]["n"] == 1 and m["hdr"]["N"] == X.D_COUNTS[k], (k, s, d, m["hdr"])
        big_at |= {r["t"] for r in m["recs"] if r["len"] > 1024}
        last_pieces.add((m["recs"][-1]["len"] + 15) // 16)
    assert {63, 64} <= big_at  # the whole-wave path at the last lane of a task and at the first of the next
    # the last record of a region at every piece count up to five that the cycle has (no length of it
    # is a single piece), so the speculative loads stop at the end of the data section
    assert {0, 2, 3, 4, 5} <= last_pieces and sorted({(ln + 15) // 16 for ln in X.D_CYCLE}) == [0, 2, 3, 4, 5, 7, 65]
    for r in range(sc.world):  # every follower receives two sources
        assert sum(1 for s in range(sc.world) if s != r and sc.pair_list(s, r)) == 2
