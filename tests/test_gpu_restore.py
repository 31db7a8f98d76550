"""rmq_restore on the GPU (FORMAT.md §11): parity with the oracle's retained windows, a device
buffer, one refusal per damage class, the every-byte sweep, padding that keeps the CRC, the host
checks, the tier round trip against tier.replay, and a world of three ranks that restart from their
windows (driven by world_script.run_gpu: threads per rank, a barrier timeout). Every expected row,
state, ring byte and index entry comes from the oracle or from the host model (tests/restore_util.py,
pinned to the oracle on the CPU by tests/test_restore_model.py), never from rmq_restore."""
import os

import numpy as np
import pytest

import parity as P
import repair_util as R
import restore_util as M
import scrub_util as U
from repl_sim import rank_cfg
from ripplemq_amd import _abi as A
from ripplemq_amd import tier as T
from ripplemq_amd.engine import Engine, EngineConfig, EngineError, LocalHub
from ripplemq_amd.sharding import rank_view
from ripplemq_amd.workload import Batch, StreamSpec, make_batch
from world_script import run_gpu, run_oracle

pytestmark = pytest.mark.gpu

OK, ECORRUPT, EINVAL, ENOSPC, ENOPART = A.RMQ_OK, A.RMQ_ECORRUPT, A.RMQ_EINVAL, A.RMQ_ENOSPC, A.RMQ_ENOPART


def _row(r):
    return (int(r["status"]), int(r["records"]), int(r["bytes"]), int(r["bad_offset"]), int(r["bad_kind"]))


def _models(cfg, wins, slots=None):
    RF = cfg.replication_factor
    return {p: M.model(run, tab, it, cfg.segment_bytes, cfg.index_interval, range(RF) if slots is None else slots, RF)
            for p, (run, tab, it) in wins.items()}


def _same_as_oracle(B, O, cfg):
    sb, so = R.snapshot(B, cfg), R.snapshot(O, cfg)
    S = cfg.segment_bytes
    for p in so:
        (stb, eb, rb), (sto, eo, ro) = sb[p], so[p]
        for f in M.STATE_FIELDS:
            assert stb[f] == sto[f], (p, f, stb[f], sto[f])
        at = np.arange(sto["log_start_pos"], sto["log_end_pos"]) % S
        for r in ro:
            assert np.array_equal(rb[r][at], ro[r][at]), (p, r)
        assert np.array_equal(eb, eo), (p, "index", eb, eo)


def _restore_and_continue(oracle_mod, cfg, batches, more, how):
    n = cfg.num_partitions
    with oracle_mod.OracleEngine(cfg) as O, Engine(cfg) as B:
        M.fill(O, batches)
        wins = {p: M.window(O, cfg, p) for p in range(n)}
        want = _models(cfg, wins)
        order = [(5 * k + 3) % n for k in range(n)]  # unsorted pidx
        assert sorted(order) == list(range(n)) and order != sorted(order)
        if how == "one_call":
            items, buf, tab = M.pack(wins, order=order)
            rows = B.restore(items, buf, tab)
            assert B.last_restore_rc == OK
            got = {int(items["pidx"][i]): _row(rows[i]) for i in range(n)}
        elif how == "device":
            items, buf, tab = M.pack(wins, order=order)
            d = B.device_alloc(buf.size)
            try:
                B.h2d(d, buf)
                rows = B.restore(items, d, tab, mem=A.RMQ_MEM_DEVICE, buf_bytes=buf.size)
            finally:
                B.device_free(d)
            got = {int(items["pidx"][i]): _row(rows[i]) for i in range(n)}
        else:
            got = {}
            for p in order:
                items, buf, tab = M.pack({p: wins[p]})
                got[p] = _row(B.restore(items, buf, tab)[0])
        assert got == {p: want[p]["row"] for p in want}, (got, want)
        for p in range(n):
            M.assert_installed(B, cfg, p, want[p])
        _same_as_oracle(B, O, cfg)
        rows = B.scrub()
        assert B.last_scrub_rc == OK
        U.assert_clean(rows, B, cfg)  # records_ok = RF x records
        # the same further batches on both, compared as every parity scenario is
        ops = [("append", Batch(*b)) for b in more]
        pidx = np.arange(n, dtype=np.uint32)
        starts = np.array([O.state(p)["log_start_offset"] for p in range(n)], np.uint64)
        ops.insert(0, ("consumer_commit", pidx, np.zeros(n, np.uint32), starts))
        ops.insert(1, ("fetch", pidx, np.zeros(n, np.uint32), np.full(n, 7, np.uint32)))
        P.run_ops(B, O, cfg, ops)
        st = [O.state(p) for p in range(n)]
        live = [p for p in range(n) if st[p]["log_end_offset"] > st[p]["log_start_offset"]]
        assert all(st[p]["log_start_offset"] > int(wins[p][2]["first_offset"][0]) for p in live), "retention ran again"
        now = np.array([s["log_start_offset"] for s in st], np.uint64)
        P.run_ops(B, O, cfg, [("consumer_commit", pidx, np.ones(n, np.uint32), now),
                              ("fetch", pidx, np.ones(n, np.uint32), np.full(n, 100, np.uint32))])
        U.assert_clean(B.scrub(), B, cfg)


@pytest.mark.parametrize("how", ["one_call", "per_partition"])
def test_parity_main(oracle_mod, how):
    _restore_and_continue(oracle_mod, M.cfg_main(), M.batches_main(), M.more_main(), how)


def test_parity_large_records(oracle_mod):
    _restore_and_continue(oracle_mod, M.cfg_big(), M.batches_big(), M.more_big(), "one_call")


def test_device_buffer(oracle_mod):
    _restore_and_continue(oracle_mod, M.cfg_main(), M.batches_main(), M.more_main(), "device")


def test_empty_logs_at_nonzero_offsets():
    """An empty run restarts an empty log; no append can leave one above offset 0, so the expected
    state is the model's. On an interval multiple the one index entry is written (§10 needs it)."""
    cfg = M.cfg_main()
    I = cfg.index_interval
    with Engine(cfg) as B:
        wins = {2: (np.zeros(0, np.uint8), np.zeros(1, np.uint64), M.item(2, 100, 100 * I, 0, 0)),
                6: (np.zeros(0, np.uint8), np.zeros(1, np.uint64), M.item(6, 7, 3 * I + 16, 0, 0))}
        want = _models(cfg, wins)
        assert len(want[2]["index"][1]) == 1 and len(want[6]["index"][1]) == 0
        items, buf, tab = M.pack(wins)
        rows = B.restore(items, buf, tab)
        assert [_row(r) for r in rows] == [want[2]["row"], want[6]["row"]]
        for p in wins:
            M.assert_installed(B, cfg, p, want[p])
        U.assert_clean(B.scrub(), B, cfg)
        offs, st = B.append(np.array([2, 6, 2], np.uint32), np.array([10, 300, 0], np.uint32), np.arange(310, dtype=np.uint8))
        assert st["appended"] == 3 and offs.tolist() == [100, 7, 101]
        assert B.state(6)["log_end_pos"] == 3 * I + 16 + 16 + 304
        U.assert_clean(B.scrub(), B, cfg)


# ---- refusals
@pytest.fixture(scope="module")
def main_windows(oracle_mod):
    cfg = M.cfg_main()
    with oracle_mod.OracleEngine(cfg) as O:
        M.fill(O, M.batches_main())
        return cfg, {p: M.window(O, cfg, p) for p in range(cfg.num_partitions)}


@pytest.mark.parametrize("what", R.CLASSES1 + M.TABLE_CLASSES)
def test_refusal_classes(main_windows, what):
    cfg, wins = main_windows
    p = 0 if what == "straddle" else 1
    run, tab, it = wins[p]
    brun, btab = M.class_damage(run, tab, it, cfg.segment_bytes, what)
    bad = dict(wins)
    bad[p] = (brun, btab, it)
    want = _models(cfg, bad)
    assert want[p]["row"][0] == ECORRUPT and M.host_refuses(brun, btab, it)
    with Engine(cfg) as B:
        before = M.pristine_snapshot(B, cfg, p)
        items, buf, rp = M.pack(bad, order=[3, 1, 0, 7, 2, 6, 5, 4])
        for dry in (True, False):
            rows = B.restore(items, buf, rp, dry_run=dry)
            assert B.last_restore_rc == ECORRUPT
            got = {int(items["pidx"][i]): _row(rows[i]) for i in range(len(items))}
            assert got == {q: want[q]["row"] for q in want}, (what, dry, got[p], want[p]["row"])
            M.assert_pristine(B, cfg, p, before)
            if dry:  # nothing changed anywhere
                assert all(B.state(q)["log_end_offset"] == 0 for q in wins)
        for q in wins:  # the other items of the call are installed and scrub clean
            if q != p:
                M.assert_installed(B, cfg, q, want[q])
        U.assert_clean(B.scrub(), B, cfg)
        good = _models(cfg, {p: wins[p]})[p]
        items, buf, rp = M.pack({p: wins[p]})
        assert _row(B.restore(items, buf, rp)[0]) == good["row"]
        M.assert_installed(B, cfg, p, good)
        U.assert_clean(B.scrub(), B, cfg)


SWEEP_LENS = (0, 5, 16, 17, 100, 239, 240, 33, 64, 1, 130)  # 1,104 record bytes, one empty payload
SWEEP_SEED = 1500  # no flip of this run leaves a record whose CRC32C still matches (asserted per flip)


def test_every_byte_sweep(oracle_mod):
    cfg = M.cfg_main()
    p = 4
    with oracle_mod.OracleEngine(cfg) as O:
        M.fill(O, [M._batch(np.random.default_rng(SWEEP_SEED), [(p, n) for n in SWEEP_LENS])])
        run, tab, it = M.window(O, cfg, p)
    assert run.size == 1104 and len(tab) == len(SWEEP_LENS) + 1
    S, I, RF = cfg.segment_bytes, cfg.index_interval, cfg.replication_factor
    with Engine(cfg) as B:
        before = M.pristine_snapshot(B, cfg, p)
        tb = tab.view(np.uint8)
        for k in range(run.size + tb.size):
            brun, btab = run.copy(), tab.copy()
            if k < run.size:
                brun[k] ^= 0x5A
            else:
                btab.view(np.uint8)[k - run.size] ^= 0x5A
            assert M.host_refuses(brun, btab, it), k  # a bad test input, not an engine failure
            want = M.model(brun, btab, it, S, I, range(RF), RF)["row"]
            got = _row(B.restore(it, brun, btab)[0])
            assert got == want and got[0] == ECORRUPT, (k, got, want)
            M.assert_pristine(B, cfg, p, before)
        good = M.model(run, tab, it, S, I, range(RF), RF)
        assert _row(B.restore(it, run, tab)[0]) == good["row"]
        M.assert_installed(B, cfg, p, good)
        U.assert_clean(B.scrub(), B, cfg)


@pytest.mark.parametrize("ln", [17, 5000])  # a lane's record, and one the whole wave folds
def test_crc_consistent_padding_is_refused(oracle_mod, ln):
    """Padding bytes chosen so that the CRC32C over the record's zero-padded pieces still matches:
    only the zero-padding rule itself refuses the record (every flip of the sweep also breaks the CRC)."""
    cfg, p = M.cfg_big(), 2
    with oracle_mod.OracleEngine(cfg) as O:
        M.fill(O, [M._batch(np.random.default_rng(1600), [(p, 40), (p, ln), (p, 7)])])
        run, tab, it = M.window(O, cfg, p)
    brun, at, pad = M.consistent_padding(run, tab, 1, oracle_mod.crc32c)
    assert pad >= 8 and brun[at] != 0 and (brun != run).sum() <= pad and M.host_refuses(brun, tab, it)
    S, I, RF = cfg.segment_bytes, cfg.index_interval, cfg.replication_factor
    want = M.model(brun, tab, it, S, I, range(RF), RF)["row"]
    assert want == (ECORRUPT, 0, 0, 1, M.CRC)
    with Engine(cfg) as B:
        before = M.pristine_snapshot(B, cfg, p)
        assert _row(B.restore(it, brun, tab)[0]) == want
        M.assert_pristine(B, cfg, p, before)
        good = M.model(run, tab, it, S, I, range(RF), RF)
        assert _row(B.restore(it, run, tab)[0]) == good["row"]
        M.assert_installed(B, cfg, p, good)


def test_host_checks(main_windows):
    cfg, wins = main_windows
    S, n = cfg.segment_bytes, cfg.num_partitions
    run, tab, it = wins[5]
    nb, cnt = run.size, len(tab) - 1
    big = np.zeros(S + 16, np.uint8)

    def var(**kw):
        x = it.copy()
        for k, v in kw.items():
            x[k] = v
        return x

    cases = [  # (item, buf, table, status)
        (var(pidx=n), run, tab, ENOPART),
        (var(bytes=S + 16, count=1, commit=1), big, np.array([0, S + 16], np.uint64), ENOSPC),
        (var(first_pos=8), run, tab, EINVAL),
        (var(buf_pos=8), np.concatenate([run, run[:16]]), tab, EINVAL),
        (var(bytes=nb - 8), run, tab, EINVAL),
        (var(buf_pos=16), run, tab, EINVAL),            # the run leaves the buffer
        (var(buf_pos=1 << 62), run, tab, EINVAL),
        (var(table_start=1), run, tab, EINVAL),         # the table leaves rec_pos
        (var(table_start=(1 << 64) - 1), run, tab, EINVAL),
        (var(count=nb // 16 + 1), run, np.zeros(nb // 16 + 2, np.uint64), EINVAL),
        (var(count=0), run, tab, EINVAL),               # no records, but bytes
        (var(commit=int(it["first_offset"][0]) + cnt + 1), run, tab, EINVAL),
        (var(first_offset=5, commit=4), run, tab, EINVAL),
        (var(flags=1), run, tab, EINVAL),
        (var(first_offset=(1 << 59) - 1, commit=(1 << 59) - 1), run, tab, EINVAL),
        (var(first_pos=(1 << 59) - 16), run, tab, EINVAL),
    ]
    with Engine(cfg) as B:
        zero = B.state(5)
        for k, (x, buf, rp, status) in enumerate(cases):
            rows = B.restore(x, buf, rp)
            assert B.last_restore_rc == status and _row(rows[0]) == (status, 0, 0, M.NONE, 0), (k, rows)
            assert B.state(5) == zero
        # a second item for the same partition: the first is installed; refused rows do not stop the others
        two = np.concatenate([it, var(pidx=n), it, wins[3][2]])
        two["buf_pos"][3], two["table_start"][3] = nb, len(tab)
        buf, rp = np.concatenate([run, wins[3][0]]), np.concatenate([tab, wins[3][1]])
        dry = B.restore(two, buf, rp, dry_run=True)
        assert [int(r["status"]) for r in dry] == [OK, ENOPART, EINVAL, OK] and B.last_restore_rc == ENOPART
        assert B.state(5) == zero and B.state(3)["log_end_offset"] == 0  # a dry run changes nothing
        rows = B.restore(two, buf, rp)
        assert [_row(r) for r in rows] == [_row(r) for r in dry]
        want = _models(cfg, {5: wins[5], 3: wins[3]})
        M.assert_installed(B, cfg, 5, want[5])
        M.assert_installed(B, cfg, 3, want[3])
        # a partition that already has records
        snap = R.snapshot(B, cfg, [5])
        assert _row(B.restore(it, run, tab)[0])[0] == EINVAL
        again = R.snapshot(B, cfg, [5])
        assert again[5][0] == snap[5][0] and all(np.array_equal(again[5][2][r], snap[5][2][r]) for r in range(3))
        # the call's own arguments
        lib = B.lib
        res = np.zeros(1, dtype=[("a", "<u8", 4)])
        args = (it.ctypes.data, A.RMQ_MEM_HOST, run.ctypes.data, run.size, tab.ctypes.data, len(tab))
        assert lib.rmq_restore(B.h, 1, *args, 2, res.ctypes.data) == EINVAL          # an unknown flag
        assert lib.rmq_restore(B.h, 1, None, *args[1:], 0, res.ctypes.data) == EINVAL  # no items
        assert lib.rmq_restore(B.h, 1, args[0], 7, *args[2:], 0, res.ctypes.data) == EINVAL  # an unknown mem
        assert lib.rmq_restore(B.h, 0, None, A.RMQ_MEM_HOST, None, 0, None, 0, 0, None) == OK
        U.assert_clean(B.scrub(), B, cfg)
        # a partition with no local slot
        B.set_replicas(6, np.array([1, 2, 3], np.uint32), 0)
        assert _row(B.restore(*M.pack({6: wins[6]}))[0]) == (EINVAL, 0, 0, M.NONE, 0)
        assert B.state(6)["log_end_offset"] == 0


def test_profile_region(main_windows):
    cfg, wins = main_windows
    with Engine(cfg) as B:
        B.profile(1)
        B.restore(*M.pack({0: wins[0], 1: wins[1]}), dry_run=True)
        B.restore(*M.pack({0: wins[0], 1: wins[1]}))
        calls, ms = B.profile_query(7)
        assert calls == 2 and 0 < ms < 1000


# ---- the tier
CURSOR = 3


def _tier_cfg():
    return EngineConfig(num_partitions=8, replication_factor=3, segment_bytes=8192, index_interval=256, max_consumers=4,
                        max_batch_records=256, max_batch_bytes=1 << 18)


def test_tier_round_trip(tmp_path):
    cfg = _tier_cfg()
    n = cfg.num_partitions
    root = str(tmp_path / "tier")
    spec = StreamSpec(n, 100, "uniform", size=(1, 120), config_index=96)
    pidx = np.arange(n, dtype=np.uint32)
    with Engine(cfg) as Aeng:
        log = T.DurableLog(Aeng, root, range(n), CURSOR, segment_file_bytes=4096)
        for k in range(16):
            b = make_batch(spec, k)
            assert Aeng.append(b.pidx, b.lens, b.payload)[1]["appended"] == b.n
            if k == 9:
                Aeng.become_leader(2, 2)
                Aeng.commit_consumer_offset(pidx, np.zeros(n, np.uint32), np.arange(n, dtype=np.uint64) + 3)
            if k % 2:
                log.spill()
        log.close()
        ends = [Aeng.state(p) for p in range(n)]
        assert all(s["log_end_pos"] > cfg.segment_bytes and s["log_start_offset"] > 0 for s in ends), "the rings wrapped"
    with Engine(cfg) as B, Engine(cfg) as Ceng:
        rb = T.restore(root, B, range(n), max_call_bytes=3 * cfg.segment_bytes)  # several calls
        rc = T.replay(root, Ceng, range(n), batch_records=64)
        assert (rb["partitions"], rb["terms"], rb["offset_rows"]) == (rc["partitions"], rc["terms"], rc["offset_rows"])
        assert 0 < rb["records"] < rc["records"]  # the retained windows only
        S = cfg.segment_bytes
        for p in range(n):
            sb, sc = B.state(p), Ceng.state(p)
            for f in ("log_end_offset", "log_end_pos", "commit", "high_watermark", "term", "voted_term", "voted_for"):
                assert sb[f] == sc[f] == ends[p][f], (p, f, sb[f], sc[f], ends[p][f])
            assert sb["log_start_pos"] <= sc["log_start_pos"] and sb["log_end_pos"] - sb["log_start_pos"] <= S
            at = np.arange(max(sb["log_start_pos"], sc["log_start_pos"]), sb["log_end_pos"]) % S
            for r in range(cfg.replication_factor):
                assert np.array_equal(B.read_segment(r, p)[at], Ceng.read_segment(r, p)[at]), (p, r)
            assert np.array_equal(B.consumer_offsets(p), Ceng.consumer_offsets(p))
        assert B.state(2)["term"] == 2 and int(B.consumer_offsets(5)[0]) == 8
        U.assert_clean(B.scrub(), B, cfg)
        # fetches from the same committed consumer offsets
        at = np.array([max(B.state(p)["log_start_offset"], Ceng.state(p)["log_start_offset"]) + 1 for p in range(n)], np.uint64)
        for e in (B, Ceng):
            e.commit_consumer_offset(pidx, np.ones(n, np.uint32), at)
        fb, fc = (e.fetch(pidx, np.ones(n, np.uint32), np.full(n, 20, np.uint32)) for e in (B, Ceng))
        assert fb[0] == fc[0] == OK and np.array_equal(fb[1], fc[1]) and np.array_equal(fb[2][:fb[3]], fc[2][:fc[3]])
        assert int(fb[1]["count"].min()) > 0
        # further batches get the same offsets on both
        for k in range(16, 19):
            b = make_batch(spec, k)
            ob, oc = B.append(b.pidx, b.lens, b.payload), Ceng.append(b.pidx, b.lens, b.payload)
            assert ob[1] == oc[1] and np.array_equal(ob[0], oc[0])
        # a consumer below B's window: RMQ_EOFFSET, and the tier's files serve it
        B.commit_consumer_offset(pidx, np.full(n, 2, np.uint32), np.zeros(n, np.uint64))
        rc2, res, _, _ = B.fetch(pidx, np.full(n, 2, np.uint32), np.full(n, 5, np.uint32))
        assert np.all(res["status"] == A.RMQ_EOFFSET)
        tier = T.DurableLog(B, root, range(n), CURSOR)
        cnt, img = tier.read_images(0, 0, 5)
        assert cnt == 5 and [o for o, _, _ in T.split_records(img)] == [0, 1, 2, 3, 4]
        tier.close()
    # files that start above offset 0 need the caller's base position
    f1 = T._PartitionFiles(root, 1, 1 << 62)
    first, base = f1.seg_first[1], f1.seg_pos[1]
    assert first > 0 and base > 0 and int(f1.pos[-1]) - base <= cfg.segment_bytes  # what is left fits the ring
    os.remove(os.path.join(root, "p000001", f"{0:020d}.seg"))
    with Engine(cfg) as D:
        with pytest.raises(EngineError) as ex:
            T.restore(root, D, [1])
        assert ex.value.status == EINVAL and D.state(1)["log_end_offset"] == 0
        assert T.restore(root, D, [1], base_pos={1: base})["partitions"] == 1
        sd = D.state(1)
        for f in ("log_end_offset", "log_end_pos", "commit", "high_watermark"):
            assert sd[f] == ends[1][f], (f, sd[f], ends[1][f])
        assert (sd["log_start_offset"], sd["log_start_pos"]) == (first, base)  # the files' first record, at the caller's position
        rows = D.scrub(1, 1)
        assert D.last_scrub_rc == OK and int(rows["records_ok"][0]) == 3 * (sd["log_end_offset"] - sd["log_start_offset"])


# ---- a world of three restarts
WORLD_BASE = dict(num_partitions=1, replication_factor=3, segment_bytes=1 << 13, index_interval=256,
                  max_batch_records=1024, max_batch_bytes=1 << 18, pipeline_depth=2, max_consumers=4)


def test_world_of_three_restarts(oracle_mod):
    world, ppr = 3, 2
    views = [rank_view(r, world, ppr, 3) for r in range(world)]
    cfgs = [rank_cfg(EngineConfig(**WORLD_BASE), views[r], r) for r in range(world)]
    spec = StreamSpec(ppr, 60, "uniform", size=(1, 100), config_index=95)

    def rounds(k0, k1):
        return [("round", {r: [make_batch(spec, 1000 * r + 10 * k + j) for j in range(2)] for r in range(world)})
                for k in range(k0, k1)]

    leads = ("lead", {r: [(p, 2) for p in range(len(views[r].gp))
                          if views[r].ranks[p][views[r].leader_slot[p]] == r] for r in range(world)})
    before, after = rounds(0, 5), [leads] + rounds(5, 7)
    local = [lambda p, r=r: [s for s in range(3) if views[r].ranks[p][s] == r] for r in range(world)]
    hub, engs, wins = LocalHub(world), [Engine(c) for c in cfgs], []
    try:
        run_gpu(engs, hub, views, before, timeout=60)
        for r in range(world):
            nloc = len(views[r].gp)
            wins.append({p: M.window(engs[r], cfgs[r], p, slot=local[r](p)[0]) for p in range(nloc)})
            assert any(engs[r].state(p)["log_start_offset"] > 0 for p in range(nloc)), "retention has run"
    finally:
        for e in engs:
            e.close()
        hub.close()
    hub, engs, oras = LocalHub(world), [Engine(c) for c in cfgs], []
    try:
        for r in range(world):  # restore every partition held, led and followed, before attaching
            rows = engs[r].restore(*M.pack(wins[r]))
            assert engs[r].last_restore_rc == OK and np.all(rows["records"] == [int(w[2]["count"][0]) for w in wins[r].values()])
        got = run_gpu(engs, hub, views, after, timeout=60)  # attach, the same placement, term 2, two rounds
        assert all(s == OK for r in range(world) for s in got[0][r])
        oras = [oracle_mod.OracleEngine(c) for c in cfgs]
        run_oracle(oras, views, before + after)  # the same script without the restart
        for r in range(world):
            cfg = cfgs[r]
            for p in range(len(views[r].gp)):
                sg, so = engs[r].state(p), oras[r].state(p)
                for f in ("log_start_offset", "log_start_pos", "log_end_offset", "log_end_pos", "commit", "high_watermark"):
                    assert sg[f] == so[f], (r, p, f, sg[f], so[f])
                for s in local[r](p):
                    assert np.array_equal(P.ring_window(engs[r], cfg, s, p, sg), P.ring_window(oras[r], cfg, s, p, so)), (r, p, s)
            sg, so = R.snapshot(engs[r], cfg, slots=local[r]), R.snapshot(oras[r], cfg, slots=local[r])
            assert all(np.array_equal(sg[p][1], so[p][1]) for p in so), (r, "index")
            stats = engs[r].replication_stats()
            # a restored follower continues its leader's log: no catch-up, no rebase, no refusal
            assert stats["catchup_entries"] == 0 and stats["refused_log"] == 0 and stats["refused_crc"] == 0, (r, stats)
            assert stats["records_ingested"] > 0
        # with a transport attached the call is refused
        with pytest.raises(EngineError) as ex:
            engs[0].restore(*M.pack({0: wins[0][0]}))
        assert ex.value.status == EINVAL
    finally:
        for o in oras:
            o.close()
        for e in engs:
            e.close()
        hub.close()
