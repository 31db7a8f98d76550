"""RMQ_FETCH_VERIFY on the GPU (FORMAT.md §10): with the flag a clean fetch is bit for bit the
fetch without it; a slice holding a flipped byte is refused (RMQ_ECORRUPT, count 0, its place in
the output kept) and commits nothing, while every other request of the call is untouched."""
import numpy as np
import pytest

import scrub_util as U
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, parse_records
from ripplemq_amd.state_machine import MessageBatchReadRequest, PartitionBroker, PartitionDirectory

pytestmark = pytest.mark.gpu

V, CM, RP = A.RMQ_FETCH_VERIFY, A.RMQ_FETCH_COMMIT, A.RMQ_FETCH_REPLICA
P, NC = 8, 4


def _commit_offsets(e, cfg):
    """Consumers at various offsets of every partition: the log start, inside, near the end, the end."""
    pidx, cons, offs = [], [], []
    for p in range(cfg.num_partitions):
        st = e.state(p)
        lo, hi = st["log_start_offset"], st["log_end_offset"]
        for c, o in enumerate((lo, lo + (hi - lo) // 3, max(lo, hi - 2), hi)):
            pidx.append(p), cons.append(c), offs.append(o)
    rc, st = e.commit_consumer_offset(np.array(pidx, np.uint32), np.array(cons, np.uint32), np.array(offs, np.uint64))
    assert rc == 0 and not st.any()


def _filled(oracle_mod=None):
    cfg = U.cfg1()
    e = Engine(cfg) if oracle_mod is None else oracle_mod.OracleEngine(cfg)
    U.fill1(e)
    _commit_offsets(e, cfg)
    return e, cfg


@pytest.fixture(scope="module")
def clean():
    e, cfg = _filled()
    yield e, cfg
    e.close()


@pytest.fixture()
def fresh():
    e, cfg = _filled()
    yield e, cfg
    e.close()


def _all_reqs(mx, flags=0):
    req = np.zeros((P * NC, 4), np.uint32)
    req[:, 0] = np.repeat(np.arange(P), NC)
    req[:, 1] = np.tile(np.arange(NC), P)
    req[:, 2] = mx
    req[:, 3] = flags
    return req


def _call(e, req, cap=1 << 17):
    """One rmq_fetch_async + poll of the rows `req` into a host buffer: (rc, rows copy, bytes, used)."""
    out = np.full(cap, 0xEE, np.uint8)
    tk = e.fetch_async(None, None, None, out=out, req=req.copy())
    rc, res, used = e.fetch_poll(tk, wait=True)
    return rc, res.copy(), out, used


@pytest.mark.parametrize("mx", [1, 10, 1024])
def test_flag_on_clean_logs_changes_nothing(clean, oracle_mod, mx):
    e, cfg = clean
    pidx, cons = np.repeat(np.arange(P), NC), np.tile(np.arange(NC), P)
    # synchronous, host output
    rc0, res0, b0, u0 = e.fetch(pidx, cons, np.full(P * NC, mx))
    rc1, res1, b1, u1 = e.fetch(pidx, cons, np.full(P * NC, mx), verify=True)
    assert (rc0, u0) == (rc1, u1) == (A.RMQ_OK, int(res0["bytes"].sum())) and u0 > 0
    assert np.array_equal(res0, res1) and np.array_equal(b0, b1)
    assert int(res0["count"].max()) == min(mx, int(res0["count"].max())) and (res0["status"] == 0).all()
    ora, _ = _filled(oracle_mod)  # the oracle's fetch of the same state
    try:
        rco, reso, bo, uo = ora.fetch(pidx, cons, np.full(P * NC, mx))
    finally:
        ora.close()
    assert (rco, uo) == (rc1, u1) and np.array_equal(reso, res1) and np.array_equal(bo[:uo], b1[:u1])
    # asynchronous, host output
    rca, resa, outa, ua = _call(e, _all_reqs(mx, V))
    assert (rca, ua) == (rc0, u0) and np.array_equal(resa, res0) and np.array_equal(outa[:ua], b0[:u0])
    assert (outa[ua:] == 0xEE).all()
    # device output, ordinary and page-locked rows, synchronous and asynchronous
    d_out = e.device_alloc(1 << 17)
    try:
        for pinned in (False, True):
            req, res = e.fetch_rows(P * NC) if pinned else (np.zeros((P * NC, 4), np.uint32), np.zeros(P * NC, FETCH_RES_DTYPE))
            req[:] = _all_reqs(mx, V)
            for asyn in (False, True):
                e.h2d(d_out, np.zeros(1 << 17, np.uint8))
                res[:] = np.zeros(1, FETCH_RES_DTYPE)[0]
                if asyn:
                    tk = e.fetch_async(None, None, None, d_out=d_out, out_cap=1 << 17, req=req, res=res, pinned_rows=pinned)
                    rcd, resd, ud = e.fetch_poll(tk, wait=True)
                else:
                    rcd, resd, ud = e.fetch_device(None, None, None, d_out, 1 << 17, req=req, res=res, pinned_rows=pinned)
                got = np.empty(1 << 17, np.uint8)
                e.d2h(got, d_out)
                assert (rcd, ud) == (rc0, u0) and np.array_equal(resd, res0), (pinned, asyn)
                assert np.array_equal(got[:ud], b0[:u0]) and not got[ud:].any(), (pinned, asyn)
    finally:
        e.device_free(d_out)


def _slice_records(e, cfg, p, consumer, mx):
    """(consumer offset, the retained records [(offset, position, len)] of its next slice)."""
    off = int(e.consumer_offsets(p)[consumer])
    recs = U.host_walk(e, cfg, 0, p)[2]
    return off, [x for x in recs if off <= x[0] < off + mx]


def _four(flags_a, flags_cd, mx=6):
    # A: partition 3 consumer 1; B: the same records without the flag (consumer 1's offset is
    # committed to consumer 2 first); C, D: other partitions
    req = np.zeros((4, 4), np.uint32)
    req[:, 0] = (3, 3, 1, 2)
    req[:, 1] = (1, 2, 1, 1)
    req[:, 2] = mx
    req[:, 3] = (flags_a, 0, flags_cd, flags_cd)
    return req


def _same_offset_for_b(e):
    a_off = int(e.consumer_offsets(3)[1])
    rc, st = e.commit_consumer_offset(np.array([3], np.uint32), np.array([2], np.uint32), np.array([a_off], np.uint64))
    assert rc == 0 and not st.any()
    return a_off


def test_refusal_touches_one_request(fresh):
    e, cfg = fresh
    S = cfg.segment_bytes
    a_off = _same_offset_for_b(e)
    rc0, res0, out0, u0 = _call(e, _four(V, V))
    assert rc0 == A.RMQ_OK and (res0["status"] == 0).all() and (res0["count"] == 6).all(), res0
    assert int(res0["bytes"][0]) == int(res0["bytes"][1])  # A and B: the same records
    _, recs = _slice_records(e, cfg, 3, 1, 6)
    rec = next(x for x in recs[1:] if x[2] > 0)
    delta = 16 + rec[2] // 2
    e.fault_flip_ring(0, 3, (rec[1] + delta) % S)  # the lowest local replica: the one the gather reads
    rc1, res1, out1, u1 = _call(e, _four(V, V))
    assert (rc1, u1) == (A.RMQ_OK, u0)
    a0, a1 = res0[0], res1[0]
    assert int(a1["status"]) == A.RMQ_ECORRUPT and int(a1["count"]) == 0, a1
    assert (int(a1["start_offset"]), int(a1["out_pos"]), int(a1["bytes"])) == \
        (a_off, int(a0["out_pos"]), int(a0["bytes"])) == (int(a0["start_offset"]), 0, int(a0["bytes"]))
    assert np.array_equal(res1[1:], res0[1:])  # B, C and D exactly as without the flip
    # A's range of a host output is left as it was; B carries the flipped byte (it asked for no check);
    # C and D are byte for byte the same
    na = int(a0["bytes"])
    assert (out1[:na] == 0xEE).all()
    want = out0.copy()
    want[:na] = 0xEE
    want[int(res0["out_pos"][1]) + (rec[1] - recs[0][1]) + delta] ^= 0x5A
    assert np.array_equal(out1, want)


def test_read_then_commit_skips_the_refused_request(fresh):
    e, cfg = fresh
    S = cfg.segment_bytes
    a_off = _same_offset_for_b(e)
    _, recs = _slice_records(e, cfg, 3, 1, 6)
    rec = next(x for x in recs if x[2] > 0)
    e.fault_flip_ring(0, 3, (rec[1] + 16) % S)
    before = {p: e.consumer_offsets(p).copy() for p in (1, 2, 3)}
    rc, res, _, _ = _call(e, _four(V | CM, V | CM))
    assert rc == A.RMQ_OK and [int(x) for x in res["status"]] == [A.RMQ_ECORRUPT, 0, 0, 0], res
    after = {p: e.consumer_offsets(p).copy() for p in (1, 2, 3)}
    assert np.array_equal(after[3], before[3])  # A committed nothing (and B never asked)
    for k, p in ((2, 1), (3, 2)):  # C and D advanced as RMQ_FETCH_COMMIT alone advances them
        want = before[p].copy()
        want[1] = int(res["start_offset"][k]) + int(res["count"][k])
        assert int(res["count"][k]) == 6 and np.array_equal(after[p], want), (p, after[p], want)
    # without the flag the old behaviour: the corrupt slice is served and committed
    rc, res, _, _ = _call(e, _four(CM, 0))
    assert rc == A.RMQ_OK and int(res["status"][0]) == 0 and int(res["count"][0]) == 6
    assert int(e.consumer_offsets(3)[1]) == a_off + 6


@pytest.mark.parametrize("what", ["len_same_size", "len_shorter", "offset"])
def test_header_flips_in_the_slice(fresh, what):
    e, cfg = fresh
    S = cfg.segment_bytes
    # consumer 0 of partition 3 stands at the log start: a long slice with the 241-byte record inside
    off, recs = _slice_records(e, cfg, 3, 0, 12)
    rec = next(x for x in recs[1:-2] if x[2] == 241)
    at, mask = {"len_same_size": (8, 0x02),   # 241 -> 243: the same 16 pieces, another CRC and padding
                "len_shorter": (8, 0x01),     # 241 -> 240: one piece shorter, the framing breaks
                "offset": (0, 0x5A)}[what]
    req = np.zeros((3, 4), np.uint32)  # two unflagged neighbours first, the flagged request last
    req[:, 0] = (1, 2, 3)
    req[:, 2] = (4, 4, 12)
    req[2, 3] = V
    d_out = e.device_alloc(1 << 16)
    try:
        def run():
            e.h2d(d_out, np.full(1 << 16, 0xEE, np.uint8))
            rc, res, used = e.fetch_device(None, None, None, d_out, 1 << 16, req=req.copy())
            got = np.empty(1 << 16, np.uint8)
            e.d2h(got, d_out)
            return rc, res.copy(), got, used
        rc0, res0, got0, u0 = run()
        assert rc0 == A.RMQ_OK and (res0["status"] == 0).all() and int(res0["count"][2]) == 12
        e.fault_flip_ring(0, 3, (rec[1] + at) % S, mask)
        rc1, res1, got1, u1 = run()
    finally:
        e.device_free(d_out)
    r = res1[2]
    print(what, "clean", res0[2], "flipped", r)
    assert rc1 == A.RMQ_OK and int(r["status"]) == A.RMQ_ECORRUPT and int(r["count"]) == 0, r
    assert np.array_equal(res1[:2], res0[:2]) and int(r["out_pos"]) == int(res0["out_pos"][2])
    assert int(r["start_offset"]) == off
    if what != "len_shorter":  # (a shorter record moves the end the resolve finds by walking the headers)
        assert int(r["bytes"]) == int(res0["bytes"][2]) and u1 == u0
    lo, hi = int(r["out_pos"]), int(r["out_pos"]) + int(r["bytes"])
    assert hi <= 1 << 16
    assert np.array_equal(got1[:lo], got0[:lo])  # nothing outside the refused request's range differs
    assert (got1[max(hi, u0):] == 0xEE).all() and (got0[u0:] == 0xEE).all()
    if hi >= u0:
        assert np.array_equal(got1[hi:], got0[hi:])


def test_replica_read_and_read_processor(fresh):
    e, cfg = fresh
    S = cfg.segment_bytes
    st = e.state(3)
    cur = st["log_start_offset"] + 1
    e.set_replica_cursor([3, 1], [cur, e.state(1)["log_start_offset"]])
    pidx, cons, mx = np.array([3, 1]), np.zeros(2), np.full(2, 5)
    rc0, res0, b0, u0 = e.fetch(pidx, cons, mx, replica=True)
    rc1, res1, b1, u1 = e.fetch(pidx, cons, mx, replica=True, verify=True)
    assert rc0 == rc1 == A.RMQ_OK and np.array_equal(res0, res1) and np.array_equal(b0, b1)
    assert int(res0["start_offset"][0]) == cur and (res0["count"] == 5).all()
    recs = [x for x in U.host_walk(e, cfg, 0, 3)[2] if cur <= x[0] < cur + 5]
    rec = next(x for x in recs if x[2] > 0)
    e.fault_flip_ring(0, 3, (rec[1] + 16) % S)
    rc2, res2, _, _ = e.fetch(pidx, cons, mx, out_cap=u0, commit=True, replica=True, verify=True)
    assert rc2 == A.RMQ_OK and [int(x) for x in res2["status"]] == [A.RMQ_ECORRUPT, 0], res2
    assert (int(res2["count"][0]), int(res2["bytes"][0]), int(res2["start_offset"][0])) == (0, int(res0["bytes"][0]), cur)
    _, res3, _, _ = e.fetch(pidx, cons, mx, replica=True)  # the refused cursor stayed, the other moved
    assert [int(x) for x in res3["start_offset"]] == [cur, int(res0["start_offset"][1]) + 5], res3
    # the read processor with verify on: a failed response for the flipped partition only
    d = PartitionDirectory({"t": P}, max_consumers=cfg.max_consumers)
    _, resw, outw, _ = _call(e, np.array([[1, 0, 5, 0]], np.uint32))
    want1 = [b for _, _, b in parse_records(outw[:int(resw["bytes"][0])])]
    br = PartitionBroker(d, engine=e, messages_as_str=False, verify=True)
    out = br.process_batch_read([MessageBatchReadRequest("c0", 40, "t", 3), MessageBatchReadRequest("c0", 5, "t", 1)])
    assert not out[0].isSuccess() and out[0].getMessages() == [] and "t-3" in out[0].getErrorMsg(), out[0]
    assert out[0].getOffset() == int(e.consumer_offsets(3)[0])
    assert out[1].isSuccess() and out[1].getErrorMsg() is None and len(out[1].getMessages()) == 5
    assert out[1].getMessages() == want1 and out[1].getOffset() == int(e.consumer_offsets(1)[0])
    plain = PartitionBroker(d, engine=e, messages_as_str=False)  # the default: served, unchecked
    assert all(x.isSuccess() for x in plain.process_batch_read([MessageBatchReadRequest("c0", 40, "t", 3)]))
