"""The argument contract of the ten fetch entry points (rmq_fetch, rmq_fetch_bytes, rmq_fetch_at,
rmq_fetch_table and their _async twins) and of rmq_fetch_poll, called through the C library.

Every refused call here is refused by host checks before anything touches the device: what is
pinned is which calls are refused, that a refused call takes no ticket and harms no ticket in
flight, and that the narrower and the wider entry points agree on a call both accept.

Rules other tests pin already (not repeated here):
  rec_pos / rec_cap without rec_row, rec_cap without rec_pos, a misaligned device rec_row, and
    rec_row[0] == 0 for a host table with n == 0            test_gpu_fetch_table.test_table_arguments
  device rows with misaligned offsets                        test_gpu_fetch_at (device rows)
  reqs and res both null with n > 0, mem == 7                test_gpu_fetch_at (entry points)
  device rows with a host output                             test_gpu_fetch_async.test_device_rows_match_host_rows
  an unknown flag bit at other rows and counts; two committing requests of one (partition, consumer)
    through rmq_fetch                                        test_gpu_fetch_async.test_fetch_commit_matches_oracle
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from ripplemq_amd import _abi as A
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine, EngineConfig

pytestmark = pytest.mark.gpu

P, NC, CAP = 4, 2, 4096
FIELDS = ("status", "start_offset", "count", "bytes", "out_pos")
KINDS = ("plain", "bytes", "at", "table")
NAME = {"plain": "rmq_fetch", "bytes": "rmq_fetch_bytes", "at": "rmq_fetch_at", "table": "rmq_fetch_table"}
EINVAL = A.RMQ_EINVAL


@pytest.fixture(scope="module")
def eng():
    cfg = EngineConfig(num_partitions=P, replication_factor=1, segment_bytes=1 << 14, index_interval=64,
                       max_consumers=NC, max_batch_records=64)
    with Engine(cfg) as e:
        lens = 5 + np.arange(12, dtype=np.uint32)
        e.append(np.arange(12) % P, lens, (np.arange(int(lens.sum())) % 251).astype(np.uint8))
        d = e.device_alloc(4 * CAP)  # device scratch of the tests: [0, CAP) output, then rows and arrays
        yield e, d
        e.device_free(d)


def _reqs(n=P, flags=0, consumer=0):
    req = np.zeros((n, 4), np.uint32)
    req[:, 0], req[:, 1], req[:, 2], req[:, 3] = np.arange(n) % P, consumer, 2, flags
    return req


def _a(x):  # an array's address, an address, or null
    return x.ctypes.data if isinstance(x, np.ndarray) else x


def issue(e, kind, asyn, req, n, mem, out, cap, res, offs=None, bud=None, tab=(None, None, 0), last=True):
    """One call of the entry point `kind`: (rc, the word its last argument points to). last=None:
    a null ticket / bytes_used."""
    fn = getattr(e.lib, NAME[kind] + ("_async" if asyn else ""))
    head = {"plain": (), "bytes": (_a(bud),), "at": (_a(offs), _a(bud)), "table": (_a(offs), _a(bud))}[kind]
    tail = (_a(tab[0]), _a(tab[1]), tab[2]) if kind == "table" else ()
    word = C.c_uint64(77)
    rc = fn(e.h, _a(req), *head, n, mem, _a(out), cap, _a(res), *tail, C.byref(word) if last else None)
    return rc, word.value


def poll(e, ticket, wait=1):
    used = C.c_uint64(77)
    return e.lib.rmq_fetch_poll(e.h, ticket, wait, C.byref(used)), used.value


def run(e, kind, asyn, *a, **k):
    """A call that must be accepted, completed: (rc, bytes_used)."""
    rc, word = issue(e, kind, asyn, *a, **k)
    if not asyn:
        return rc, word
    assert rc == A.RMQ_OK
    return poll(e, word)


def _same(res, want):
    return all(np.array_equal(res[f], want[f]) for f in FIELDS)


@pytest.fixture(scope="module")
def plain(eng):
    """The reference of the module: rmq_fetch of _reqs() into a host output (rc, res, out, used)."""
    e, _ = eng
    res, out = np.zeros(P, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8)
    rc, used = run(e, "plain", False, _reqs(), P, A.RMQ_MEM_HOST, out, CAP, res)
    assert rc == A.RMQ_OK and used == int(res["bytes"].sum()) > 0 and (res["count"] == 2).all()
    return rc, res, out, used


def _next_ticket(e):
    """The number the next accepted call takes (an empty asynchronous call takes one)."""
    rc, t = issue(e, "plain", True, None, 0, A.RMQ_MEM_HOST, None, 0, None)
    assert rc == A.RMQ_OK and poll(e, t) == (A.RMQ_OK, 0)
    return t + 1


def test_refused_arguments(eng):
    e, d = eng
    req, res, out = _reqs(), np.zeros(P, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8)
    row, pos = np.zeros(P + 1, np.uint64), np.zeros(64, np.uint64)
    d_req, d_res, d_arr = d + CAP, d + 2 * CAP, d + 3 * CAP
    host, dev = A.RMQ_MEM_HOST, A.RMQ_MEM_DEVICE
    drows = dev | A.RMQ_FETCH_DEVICE_ROWS
    e.h2d(d_req, req)
    first = _next_ticket(e)
    for asyn in (False, True):
        for kind in KINDS:
            why = (kind, asyn)
            bad = lambda *a, **k: issue(e, kind, asyn, *a, **k)[0] == EINVAL  # noqa: E731
            assert bad(None, P, host, out, CAP, res), why           # null reqs
            assert bad(req, P, host, out, CAP, None), why           # null res
            for mem in (2, 3, 2 | A.RMQ_FETCH_FILL, 0x800):         # neither host nor device
                assert bad(req, P, mem, out, CAP, res), (why, mem)
            assert bad(req, P, host, None, CAP, res), why           # out_cap without out
            assert bad(req, P, dev, d + 8, CAP, res), why           # a device output is 16-byte aligned
            assert bad(d_req, P, drows | A.RMQ_FETCH_PINNED_ROWS, d, CAP, d_res), why
            if asyn:
                assert bad(req, P, host, out, CAP, res, last=None), why  # null ticket
                assert bad(None, 0, host, None, 0, None, last=None), why
            if kind != "plain":  # device rows: their budgets are 4-byte aligned
                assert bad(d_req, P, drows, d, CAP, d_res, bud=d_arr + 2), why
        # the table's arrays, through the asynchronous call (the synchronous one: see the header)
        tb = lambda *t, mem=host, o=out: issue(e, "table", asyn, req, P, mem, o, CAP, res, tab=t)[0]  # noqa: E731
        if asyn:
            assert tb(None, pos, 64) == tb(None, None, 64) == tb(row, None, 64) == EINVAL
        assert tb(d_arr, d_arr + 1024 + 4, 8, mem=dev, o=d) == EINVAL  # a device rec_pos is 8-byte aligned
    assert _next_ticket(e) == first + 1  # none of them took a ticket


@pytest.mark.parametrize("asyn", (False, True))
def test_refused_flags(eng, plain, asyn):
    e, d = eng
    res, out = np.zeros(5, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8)
    table = e.consumer_table().copy()
    first = _next_ticket(e)
    for at in (0, 4):  # an unknown bit: in the four-wide scan, and in its tail
        req = _reqs(5)
        req[at, 3] |= 4
        assert issue(e, "plain", asyn, req, 5, A.RMQ_MEM_HOST, out, CAP, res)[0] == EINVAL, at
    # two committing requests of one (partition, consumer); two committing replica reads of one
    # partition under different consumer keys (one replica cursor per partition)
    for flags, cons in ((A.RMQ_FETCH_COMMIT, (1, 1)), (A.RMQ_FETCH_COMMIT | A.RMQ_FETCH_REPLICA, (0, 1))):
        req = _reqs(3, flags)
        req[:, 0], req[:, 1] = (2, 1, 2), (cons[0], 0, cons[1])
        assert issue(e, "plain", asyn, req, 3, A.RMQ_MEM_HOST, out, CAP, res)[0] == EINVAL, flags
    assert _next_ticket(e) == first + 1
    assert np.array_equal(e.consumer_table(), table)
    # device rows are never read on the host: the unknown bit (and a commit flag) is ignored
    req, d_req, d_res = _reqs(), d + CAP, d + 2 * CAP
    req[:, 3] = 4 | A.RMQ_FETCH_COMMIT
    e.h2d(d_req, req)
    rc, used = run(e, "plain", asyn, d_req, P, A.RMQ_MEM_DEVICE | A.RMQ_FETCH_DEVICE_ROWS, d, CAP, d_res)
    got = np.zeros(P, FETCH_RES_DTYPE)
    e.d2h(got, d_res)
    assert (rc, used) == (plain[0], plain[3]) and _same(got, plain[1])
    assert np.array_equal(e.consumer_table(), table)


@pytest.mark.parametrize("asyn", (False, True))
def test_accepted_edges(eng, plain, asyn):
    e, d = eng
    host, dev = A.RMQ_MEM_HOST, A.RMQ_MEM_DEVICE
    # the size probe: rec_pos null with rec_cap 0 gives rec_row alone (RMQ_ENOSPC: words are needed)
    res, out, row = np.zeros(P, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8), np.full(P + 1, 9, np.uint64)
    rc, used = run(e, "table", asyn, _reqs(), P, host, out, CAP, res, tab=(row, None, 0))
    words = np.concatenate(([0], np.cumsum(plain[1]["count"].astype(np.uint64) + 1)))
    assert rc == A.RMQ_ENOSPC and used == plain[3] and _same(res, plain[1]) and np.array_equal(row, words)
    # a committing request of a partition that does not exist takes no part in the duplicate check:
    # the call succeeds, the row carries its own status, the valid row next to it is served
    req = _reqs(3, A.RMQ_FETCH_COMMIT, consumer=1)
    req[:, 0], req[:, 2] = (P + 3, 0, P + 3), 1
    res = np.zeros(3, FETCH_RES_DTYPE)
    before = int(e.consumer_offsets(0)[1])
    rc, used = run(e, "plain", asyn, req, 3, host, out, CAP, res)
    assert rc == A.RMQ_OK and [int(s) for s in res["status"]] == [A.RMQ_ENOPART, A.RMQ_OK, A.RMQ_ENOPART]
    assert res["count"][1] == 1 and used == res["bytes"][1] and int(e.consumer_offsets(0)[1]) == before + 1
    # n == 0: complete at once, nothing used; a table's rec_row[0] is 0, host and device
    for kind in KINDS:
        assert run(e, kind, asyn, None, 0, host, None, 0, None) == (A.RMQ_OK, 0), kind
        assert run(e, kind, asyn, None, 0, dev, None, 0, None) == (A.RMQ_OK, 0), kind
    row, pos = np.full(1, 9, np.uint64), np.zeros(8, np.uint64)
    assert run(e, "table", asyn, None, 0, host, None, 0, None, tab=(row, pos, 8)) == (A.RMQ_OK, 0) and row[0] == 0
    e.h2d(d, np.full(2, 9, np.uint64))
    assert run(e, "table", asyn, None, 0, dev, None, 0, None, tab=(d, d + 8, 1)) == (A.RMQ_OK, 0)
    got = np.ones(2, np.uint64)
    e.d2h(got, d)
    assert got[0] == 0 and got[1] == 9


def test_tickets(eng, plain):
    e, _ = eng
    host = A.RMQ_MEM_HOST
    bad = _reqs(5)
    bad[4, 3] = 8
    scratch = np.zeros(5, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8)
    first = _next_ticket(e)
    held = []
    for k in range(4):  # accepted calls take consecutive numbers; a refused call in between takes none
        res, out = np.zeros(P, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8)
        rc, t = issue(e, KINDS[k], True, _reqs(), P, host, out, CAP, res)
        assert (rc, t) == (A.RMQ_OK, first + k)
        held.append((t, res, out))
        refused = (issue(e, "plain", True, None, P, host, scratch[1], CAP, scratch[0]),       # its arguments
                   issue(e, "plain", True, bad, 5, host, scratch[1], CAP, scratch[0]))        # its flags
        assert [r[0] for r in refused] == [EINVAL, EINVAL]
    # (every slot is taken: the last refused call completed the oldest ticket before it read its flags)
    assert poll(e, first + 4) == (EINVAL, 0)  # never issued
    for t, res, out in held[::-1]:
        assert poll(e, t) == (plain[0], plain[3]) and _same(res, plain[1]) and np.array_equal(out, plain[2]), t
    for t, _, _ in held:
        assert poll(e, t) == (EINVAL, 0)  # answered once
    assert _next_ticket(e) == first + 4 + 1  # (the four, and the empty call that asked)


@pytest.mark.parametrize("asyn", (False, True))
def test_wider_entry_points_equal_the_narrower(eng, plain, asyn):
    """rmq_fetch_table with null table arrays is rmq_fetch_at, rmq_fetch_at with null offsets is
    rmq_fetch_bytes, rmq_fetch_bytes with null budgets is rmq_fetch; and with budgets given, the
    three that take them agree."""
    e, _ = eng
    bud = np.array([0, 40, 1, 0], np.uint32)
    got = {}
    for b in (None, bud):
        for kind in KINDS[(0 if b is None else 1):]:
            res, out = np.zeros(P, FETCH_RES_DTYPE), np.zeros(CAP, np.uint8)
            rc, used = run(e, kind, asyn, _reqs(), P, A.RMQ_MEM_HOST, out, CAP, res, bud=b)
            got[kind, b is None] = (rc, used, res, out)
    for (kind, nobud), (rc, used, res, out) in got.items():
        w = (plain[0], plain[3], plain[1], plain[2]) if nobud else got["bytes", False]
        assert (rc, used) == w[:2] and _same(res, w[2]) and np.array_equal(out, w[3]), (kind, nobud)
    assert got["bytes", False][1] < plain[3]  # (the budgets cut something)
