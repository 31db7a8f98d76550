"""The case tables of tests/stage1_edges_util.py without a GPU: that each holds the edge it is named
for in both kernel geometries (from the model's arithmetic alone: the sorted runs of every tile, the
hash table's probe sequences, the key widths, the flags), and that the C oracle places every record
where the model's ranks and byte prefixes say, counts the flagged records and rejects none for
space. The model and the oracle agreeing here is what makes the device comparison of
tests/test_gpu_stage1_edges.py meaningful."""
import functools

import numpy as np
import pytest

import stage1_edges_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import EngineConfig, EngineError

GEOMETRIES = tuple(U.WAVE_RECS)


@functools.lru_cache(maxsize=None)
def table(name: str) -> U.Table:
    """The tables are built once for the module (tests only read them)."""
    return U.table(name)


def tile_models(c, P):
    fl, _ = U.record_flags(c, P)
    return [U.tile_model(c, P, t, fl) for t in range(U.tiles_of(c.batch.n))]


# ---- the model's own parts --------------------------------------------------------------------

def test_model_ranks_are_stable_ranks():
    """tile_model against its definition said another way: the rank of a valid record is the number
    of valid records of its partition before it in the tile, by counting with numpy masks."""
    t = table("flags")
    c = t.groups[0][0]
    fl, bad = U.record_flags(c, t.P)
    assert bad == 0 and (fl == U.FL_NOPART).sum() == 4
    tm = U.tile_model(c, t.P, 0, fl)
    pidx, un = c.batch.pidx[:1024].astype(np.int64), U.units(c.batch.lens[:1024])
    for q in range(0, 1024, 37):
        if fl[q]:
            continue
        same = (pidx[:q] == pidx[q]) & (fl[:q] == 0)
        assert tm.rank[q] == same.sum() and tm.pre16[q] == un[:q][same].sum()
    assert sum(n for n, _ in tm.cells.values()) == (fl[:1024] == 0).sum()
    assert tm.pre[5] == c.batch.lens[:5].sum()


def test_hash_slot_formula():
    assert U.hash_slot([0, 1, 986]).tolist() == [(2654435761 >> 21) & 2047, ((2 * 2654435761) & 0xFFFFFFFF) >> 21, 2047]
    h = U.hash_slot(np.arange(65536))
    assert h.min() == 0 and h.max() == U.HT - 1 and np.bincount(h).max() == 34


def test_key_widths():
    for P, want in U.KEY_WIDTHS.items():
        assert U.key_width(P) == want, P
    assert {U.key_width(P)[1] for P in U.KEY_PS} == {0, 1, 2}
    assert [U.key_width(P)[0] for P in (255, 256, 257)] == [8, 8, 9]  # one pass to two, 8 bits to 9


# ---- every table: sizes -------------------------------------------------------------------------

@pytest.mark.parametrize("name", U.TABLES)
def test_tables_fit_their_engines(name):
    t = table(name)
    cfg = EngineConfig(**t.cfg)
    for g in t.groups:
        assert 1 <= len(g) <= cfg.pipeline_depth
        assert sum(U.tiles_of(c.batch.n) for c in g) <= min(512, cfg.pipeline_depth * U.tiles_of(cfg.max_batch_records))
        for c in g:
            assert 0 < c.batch.n <= cfg.max_batch_records and c.batch.payload.size <= cfg.max_batch_bytes
            assert c.batch.lens.max() <= 3000
            assert (c.batch.lens > 200).sum() <= 16, "a handful of large records at most"
    assert sum(c.batch.n for c in t.cases()) <= 32768


# ---- runs ---------------------------------------------------------------------------------------

def test_runs_table_lays_its_runs_where_it_says():
    t = table("runs")
    srt, shuf = t.groups[0]
    for c in (srt, shuf):
        tms = tile_models(c, t.P)
        assert len(tms) == len(U.RUN_TILES)
        for tm, (name, want) in zip(tms, U.RUN_TILES.items()):
            runs = U.sorted_runs(tm)
            assert [(a, b) for _, a, b, _ in runs] == want, (c.name, name)
            assert [k for k, *_ in runs] == U.RUN_PARTS[name]
            assert all(v == b - a for _, a, b, v in runs)  # every item valid: a cell for every run
            for geo in GEOMETRIES:
                got = U.run_edges(runs, U.WAVE_RECS[geo])
                assert U.RUN_EDGES[name][geo] <= got, f"{name} / {geo}: misses {U.RUN_EDGES[name][geo] - got}"
    # the sorted batch is in sorted order, the shuffled one is not, and both hold the same tiles
    assert all((np.diff(srt.batch.pidx[k:k + 1024].astype(int)) >= 0).all() for k in range(0, srt.batch.n, 1024))
    assert any((np.diff(shuf.batch.pidx[k:k + 1024].astype(int)) < 0).any() for k in range(0, shuf.batch.n, 1024))
    for k in range(0, srt.batch.n, 1024):
        assert np.array_equal(np.sort(srt.batch.pidx[k:k + 1024]), np.sort(shuf.batch.pidx[k:k + 1024]))
    # record sizes from 1 to 13 units, varying
    un = U.units(srt.batch.lens)
    assert un.min() == 1 and un.max() == 13 and len(np.unique(un)) == 13
    # both geometries see every edge somewhere in the table
    for geo in GEOMETRIES:
        seen = set().union(*(U.run_edges(U.sorted_runs(tm), U.WAVE_RECS[geo]) for tm in tile_models(srt, t.P)))
        assert {"starts_at_lane_63", "ends_at_lane_0", "two_whole_waves_without_head", "head_only_in_last_slot_of_wave",
                "head_only_in_first_slot_of_wave", "whole_tile", "single_item_run", "crosses_slot_in_wave",
                "crosses_wave"} <= seen, geo


def test_named_runs_cross_what_they_should():
    """The two-record runs of the first tile: [63, 65) crosses a slot inside a wave in both
    geometries; [127, 129) crosses a wave only where a wave holds 128 items; [255, 257) in both."""
    cross = lambda a, b, w: (a // U.SLOT != (b - 1) // U.SLOT, a // w != (b - 1) // w)
    assert [cross(63, 65, w) for w in (256, 128)] == [(True, False), (True, False)]
    assert [cross(127, 129, w) for w in (256, 128)] == [(True, False), (True, True)]
    assert [cross(255, 257, w) for w in (256, 128)] == [(True, True), (True, True)]
    assert set(U.WAVE_RECS.values()) == {256, 128}


# ---- nin ----------------------------------------------------------------------------------------

def test_nin_table_sizes_and_key_zero():
    t = table("nin")
    single = [g[0] for g in t.groups if len(g) == 1]
    assert sorted({c.batch.n for c in single}) == sorted(U.NIN_SIZES)
    for w in U.WAVE_RECS.values():  # one wave's records and one more or less, in both geometries
        assert {w - 1, w, w + 1} <= set(U.NIN_SIZES)
    assert {1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049} <= set(U.NIN_SIZES)
    mixes = [tuple(c.batch.n for c in g) for g in t.groups if len(g) > 1]
    assert mixes == list(U.NIN_MIXES) and all(2 <= len(m) <= 4 for m in mixes)
    assert any(a % 1024 == 0 and b % 1024 == 1 for m in mixes for a, b in zip(m, m[1:]))  # full tiles, then one record
    assert any(a % 1024 == 1 and b % 1024 == 0 for m in mixes for a, b in zip(m, m[1:]))
    # key 0's run: per size, a last tile where it holds valid records, unknown ones and junk lanes,
    # and one where it holds only unknown records and junk (no cell for partition 0)
    for n in U.NIN_SIZES:
        kinds = set()
        for c in single:
            if c.batch.n != n:
                continue
            tm = tile_models(c, t.P)[-1]
            key0 = [r for r in U.sorted_runs(tm) if r[0] == 0]
            junk = U.TILE_RECS - tm.nin
            assert len(key0) == (1 if junk or (tm.key == 0).any() else 0)
            unknown = int((tm.fl == U.FL_NOPART).sum())
            if key0:
                k, a, b, valid = key0[0]
                assert a == 0 and b - a == valid + unknown + junk
                assert (0 in tm.cells) == (valid > 0)
                kinds.add(("valid" if valid else "none", "unknown" if unknown else "-", "junk" if junk else "-"))
        assert any(k[0] == "valid" for k in kinds), n
        assert any(k[0] == "none" for k in kinds), n
        if (n - 1) % 1024 >= 3:  # (the last tile holds four records or more)
            assert any(k[0] == "none" and k[1] == "unknown" for k in kinds), n
        if n % 1024:
            assert all(k[2] == "junk" for k in kinds), n
    assert any(c.batch.n == 1 and 0 not in tile_models(c, t.P)[0].cells for c in single)  # junk lanes alone


# ---- keys ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", U.KEY_PS)
def test_keys_tables_hold_their_extremes(P):
    t = table(f"keys-P{P}")
    assert t.P == P and U.key_width(P) == U.KEY_WIDTHS[P]
    ext = t.notes["ext"]
    assert {0, P - 1} <= set(ext)
    if P == 65536:
        assert set(U.EXTREMES_65536) <= set(ext)
        digits = {(p >> 8, p & 255) for p in U.EXTREMES_65536}
        assert {(0, 0), (0, 255), (1, 0), (254, 255), (255, 0), (255, 255)} == digits
    cases = t.cases()
    if P >= 1024:
        tm = tile_models(cases[0], P)[0]
        runs = U.sorted_runs(tm)
        assert cases[0].batch.n == 1024 and len(runs) == 1024 and all(v == 1 for *_, v in runs)
        assert "every_item_a_head" in U.run_edges(runs, 256)
        assert set(ext) <= set(cases[0].batch.pidx.tolist())
        assert U.probe_tile(tm)["leaders"] == [64] * 16  # hash mode: every record its key's leader
    rep = cases[-2]
    for tm in tile_models(rep, P):  # the extremes in both tiles, partitions repeating, unknown ones at the ends
        assert set(ext) <= set(tm.cells), P
        assert max(n for n, _ in tm.cells.values()) > 1
        assert tm.fl[0] == U.FL_NOPART and tm.fl[-1] == U.FL_NOPART
    assert {P, P + 1, U.UNKNOWN} <= set(rep.batch.pidx.tolist())
    if P == 1:
        assert set(rep.batch.pidx.tolist()) == {0, 1, 2, U.UNKNOWN}


def test_big_engine_is_small():
    """The P = 65536 engine by its own configuration: ring and index bytes (the rest: util.big_cfg)."""
    cfg = EngineConfig(**U.big_cfg())
    rings = cfg.num_partitions * cfg.segment_bytes * cfg.replication_factor
    index = rings // cfg.replication_factor // cfg.index_interval * (2 * cfg.pipeline_depth + 2) * 16
    assert rings == 256 * U.MIB and index == 96 * U.MIB
    assert cfg.segment_bytes >= 4 * cfg.index_interval and table("hash").cfg == U.big_cfg()


# ---- hash ---------------------------------------------------------------------------------------

def test_hash_table_wraps_clusters_and_crowds():
    t = table("hash")
    P = t.P
    assert t.notes["most_per_h"] == 34 < U.SLOT  # 64 partitions of one h do not exist below 2^16
    tms = {c.name: tile_models(c, P)[0] for c in t.cases()}
    hs = {name: U.hash_slot(sorted(tm.cells)) for name, tm in tms.items()}
    pr = {name: U.probe_tile(tm) for name, tm in tms.items()}
    # every partition of the tile starts at slot 2047: all but the first to come wrap, whoever wins
    assert (hs["h2047"] == U.HT - 1).all() and len(hs["h2047"]) >= 30
    assert len(pr["h2047"]["wrapped"]) == len(hs["h2047"]) - 1
    assert pr["h2047"]["longest"] == len(hs["h2047"])
    # a cluster over the wrap: more keys from 2044 on than the four slots hold
    assert (hs["h2044+"] >= U.HT - 4).all() and len(hs["h2044+"]) > 100
    assert len(pr["h2044+"]["wrapped"]) >= len(hs["h2044+"]) - 4
    assert max(pr["h2044+"]["table"].values()) == U.HT - 1 and min(pr["h2044+"]["table"].values()) == 0
    assert pr["h2044+"]["longest"] > 64
    # one input slot of 64 leaders: 34 of one h (the most there are) and 30 of the h before it
    h0 = t.notes["h0"]
    assert tms["crowd"].nin == 64 and pr["crowd"]["leaders"] == [64] and pr["crowd"]["same_h"] == [34]
    assert sorted(set(hs["crowd"].tolist())) == [h0 - 1, h0] and 0 < h0 - 1 and h0 + 64 < U.HT
    # and over the wrap: 32 of h 2047 and 32 of h 2046 in one input slot
    assert pr["crowd-wrap"]["leaders"] == [64] and pr["crowd-wrap"]["same_h"] == [32]
    assert sorted(set(hs["crowd-wrap"].tolist())) == [U.HT - 2, U.HT - 1] and len(pr["crowd-wrap"]["wrapped"]) == 62
    # the mixed tile: ordinary partitions, the sets above, flagged records; it wraps as well
    m = hs["mixed"]
    assert tms["mixed"].nin == 1024 and (m == U.HT - 1).sum() >= 2 and ((m > 64) & (m < U.HT - 64)).sum() > 100
    assert pr["mixed"]["wrapped"] and (tms["mixed"].fl == U.FL_NOPART).sum() == 2
    assert max(pr["mixed"]["leaders"]) > 40
    # the slot of 64 leaders first, then further slots that find their keys in the table
    more = pr["crowd-then-more"]
    assert more["leaders"][0] == 64 and len(more["leaders"]) == 4 and more["wrapped"]
    for name, p in pr.items():  # the table's cells: one per present partition
        assert p["counts"] == tms[name].cells and set(p["table"]) == set(tms[name].cells), name
        assert len(set(p["table"].values())) == len(p["table"]), name


# ---- flags --------------------------------------------------------------------------------------

def test_flags_table_puts_flagged_records_at_the_edges_of_runs():
    t = table("flags")
    P = t.P
    (a, b, c), (d, e, f) = t.groups
    assert [x.invalid for x in (a, b, c, d, e, f)] == [False, True, False, True, False, False]
    assert all(x.poff is not None for x in (a, b, c, d, f)) and e.poff is None
    big_at = t.notes["big_at"]

    # A: unknown partitions first and last of both tiles, i.e. first and last of key 0's run
    fl, bad = U.record_flags(a, P)
    assert bad == 0 and np.flatnonzero(fl).tolist() == [0, 1023, 1024, a.batch.n - 1]
    t0, t1 = tile_models(a, P)
    r0 = U.sorted_runs(t0)[0]
    assert r0[0] == 0 and r0[3] == r0[2] - 2 and 0 in t0.cells   # key 0: valid records between two unknown ones
    r1 = U.sorted_runs(t1)[0]
    assert r1[0] == 0 and r1[3] == 0 and 0 not in t1.cells      # tile 1: two unknown records and junk only
    assert r1[2] - r1[1] == 2 + U.TILE_RECS - t1.nin
    assert t.notes["absent"] not in t0.cells and t.notes["absent"] not in t1.cells
    assert sorted(t0.big + [1024 + q for q in t1.big]) == big_at
    for q in (0, 1023, 1024, a.batch.n - 1):  # a large valid record in each flagged record's slot
        assert any(q // 64 == g // 64 for g in big_at), q

    # B: out-of-range records at the edges of their partitions' runs
    fl, bad = U.record_flags(b, P)
    tb0, tb1 = tile_models(b, P)
    assert bad == (fl == U.FL_INVALID).sum() + 1 and fl[2] == U.FL_NOPART  # record 2: unknown and out of range
    assert fl[0] == U.FL_INVALID and fl[1023] == U.FL_INVALID and fl[b.batch.n - 1] == U.FL_INVALID
    pidx = b.batch.pidx.astype(np.int64)
    p3 = np.flatnonzero(pidx[:1024] == 3)
    assert fl[p3[0]] == fl[p3[-1]] == U.FL_INVALID and (fl[p3[1:-1]] == 0).all() and len(p3) > 4
    assert tb0.cells[3][0] == len(p3) - 2 and tb0.rank[p3[1]] == 0   # the ranks do not count the flagged ones
    p7 = np.flatnonzero(pidx[:1024] == t.notes["all_invalid"])
    assert len(p7) >= 8 and (fl[p7] == U.FL_INVALID).all() and t.notes["all_invalid"] not in tb0.cells
    p11 = np.flatnonzero(pidx[:1024] == t.notes["alone"])
    assert p11.tolist() == [300] and fl[300] == U.FL_INVALID and t.notes["alone"] not in tb0.cells
    assert t.notes["alone"] in tb1.cells and t.notes["all_invalid"] not in tb1.cells
    run7 = [r for r in U.sorted_runs(tb0) if r[0] == 7][0]
    assert run7[3] == 0 and run7[2] - run7[1] == len(p7)             # a run, and no valid record in it
    # both kinds of bad range
    D = b.declared
    o, L = b.poff.astype(object), b.batch.lens.astype(object)
    inv = np.flatnonzero(fl == U.FL_INVALID)
    assert any(o[k] <= D and o[k] + L[k] == D + 1 for k in inv) and any(o[k] > D for k in inv)
    # large records: the valid ones in the list, not the one out of range (40) nor the unknown one (70)
    assert b.batch.lens[40] > 1024 and fl[40] == U.FL_INVALID and pidx[70] == U.UNKNOWN and b.batch.lens[70] > 1024
    assert sorted(tb0.big + [1024 + q for q in tb1.big]) == [q for q in big_at if q not in (40, 70)]
    for q in (0, 1023, b.batch.n - 1):
        assert any(q // 64 == g // 64 for g in big_at if g not in (40, 70)), q

    # D: one bad record, the last one, alone in its tile
    fl, bad = U.record_flags(d, P)
    assert bad == 1 and np.flatnonzero(fl).tolist() == [1024] and d.batch.n == 1025
    # F: the rule's valid edges
    fl, bad = U.record_flags(f, P)
    assert bad == 0 and not fl.any()
    assert f.batch.lens[3] == 0 and f.poff[3] == f.declared and f.batch.lens[64] == 0 and f.poff[64] == f.declared + 1
    assert int(f.poff[127]) + int(f.batch.lens[127]) == f.declared and f.batch.lens[127] > 0
    # E: packed, unknown partitions in front, large records
    assert U.record_flags(e, P)[0][:3].tolist() == [1, 1, 1] and len(tile_models(e, P)[0].big) == 2


# ---- oracle -------------------------------------------------------------------------------------

def through_oracle(O, t: U.Table):
    """Every batch of the table through the oracle, and for each the model's prediction: a valid
    record's offset is its partition's log end before the batch + the valid records of the partition
    in the batch's earlier tiles + its rank in its tile; its position likewise from the log end
    position and 16 x the byte prefixes; every other record gets none."""
    cfg = EngineConfig(**t.cfg)
    P = cfg.num_partitions
    leo, used = {}, {}
    totals = dict(records=0, appended=0, no_partition=0, invalid=0)
    with O.OracleEngine(cfg) as ora:
        for gi, g in enumerate(t.groups):
            for c in g:
                b, what = c.batch, f"{t.name} group {gi} batch {c.name}"
                fl, bad = U.record_flags(c, P)
                pay = b.payload[:U.declared_bytes(c)]
                totals["records"] += b.n
                if bad:
                    assert c.invalid, what
                    with pytest.raises(EngineError) as ex:
                        ora.append(b.pidx, b.lens, pay, c.poff)
                    assert ex.value.status == A.RMQ_EINVAL, what
                    totals["invalid"] += b.n
                    continue
                assert not c.invalid, what
                out, st = ora.append(b.pidx, b.lens, pay, c.poff)
                want = np.full(b.n, U.NONE, np.uint64)
                pos = {}
                for ti, tm in enumerate(U.tile_model(c, P, k, fl) for k in range(U.tiles_of(b.n))):
                    for q in np.flatnonzero(tm.fl == 0).tolist():
                        p = int(tm.key[q])
                        want[ti * 1024 + q] = leo.get(p, 0) + tm.rank[q]
                        pos[ti * 1024 + q] = (p, used.get(p, 0) + 16 * int(tm.pre16[q]))
                    for p, (n, u16) in tm.cells.items():
                        leo[p], used[p] = leo.get(p, 0) + n, used.get(p, 0) + 16 * u16
                assert np.array_equal(out, want), f"{what}: offsets differ at {np.flatnonzero(out != want)[:8]}"
                for k, (p, at) in list(pos.items())[::7]:
                    assert ora.record_pos(p, int(out[k])) == at, f"{what}: position of record {k}"
                nop = int((fl == U.FL_NOPART).sum())
                assert st == dict(records=b.n, appended=b.n - nop, rejected_not_leader=0, rejected_no_partition=nop,
                                  rejected_no_space=0, rejected_invalid=0), f"{what}: {st}"
                totals["appended"] += b.n - nop
                totals["no_partition"] += nop
        for p in leo:
            s = ora.state(p)
            assert (s["log_end_offset"], s["log_end_pos"]) == (leo[p], used[p]), p
        untouched = [p for p in {0, 1, P // 2, P - 1} if p < P and p not in leo]
        assert all(ora.state(p)["log_end_offset"] == 0 for p in untouched)
    return totals


@pytest.mark.parametrize("name", U.TABLES)
def test_tables_through_oracle_and_model(oracle_mod, name):
    t = table(name)
    tot = through_oracle(oracle_mod, t)
    assert tot["appended"] > 0 and tot["records"] == tot["appended"] + tot["no_partition"] + tot["invalid"]
    if name in ("nin", "flags", "hash") or name.startswith("keys"):
        assert tot["no_partition"] > 0
    if name == "flags":
        assert tot["invalid"] == sum(c.batch.n for c in t.cases() if c.invalid) > 0
    else:
        assert tot["invalid"] == 0
