"""The model of rmq_unpack (tests/unpack_util.py) on the oracle, without a GPU: on an oracle fetch its
columns and payloads are parse_records of every served row; view columns are an append batch that
reproduces the payloads; the structure checks name the row they should; and the scenarios of
tests/test_gpu_unpack.py hold every category that file claims."""
import numpy as np
import pytest

import unpack_util as M
from ripplemq_amd import _abi as A
from ripplemq_amd.engine import parse_records


@pytest.fixture(scope="module")
def ora(oracle_mod):
    e = oracle_mod.OracleEngine(M.cfg_mix())
    M.fill_mix(e)
    yield e
    e.close()


def _served(buf, res):
    return [parse_records(buf[int(r["out_pos"]):int(r["out_pos"]) + int(r["bytes"])]) if ok else []
            for r, ok in zip(res, M.owning(res))]


@pytest.mark.parametrize("mode", ["view", "packed", 1, 16, 17, 100, 128])
def test_the_model_is_parse_records_of_every_served_row(ora, mode):
    buf, res, row, pos = M.host_fetch(ora, *M.reqs_len_mix())
    m = M.model_unpack(buf, res, row, pos, mode)
    want = _served(buf, res)
    flat = [x for recs in want for x in recs]
    assert m["status"] == A.RMQ_OK and m["records"] == len(flat) == 2 * len(M.LENMIX) * M.P_MIX and m["mismatched"] == 0
    assert list(m["rec_first"]) == list(np.concatenate(([0], np.cumsum([len(x) for x in want]))))
    assert list(m["offset"]) == [o for o, _, _ in flat] and list(m["len"]) == [len(b) for _, _, b in flat]
    assert list(m["tag"]) == [r for r, recs in enumerate(want) for _ in recs]
    if isinstance(mode, str):
        assert M.payloads_of(m, buf) == [b for _, _, b in flat]
        assert m["payload_bytes"] == (0 if mode == "view" else sum(len(b) for _, _, b in flat))
    else:
        assert m["payload"].shape == (len(flat), mode) and m["payload_bytes"] == len(flat) * mode
        for j, (_, _, b) in enumerate(flat):
            assert m["payload"][j].tobytes() == b[:mode] + bytes(mode - min(len(b), mode))
        assert m["truncated"] == sum(len(b) > mode for _, _, b in flat) > 0


def test_view_columns_are_an_append_batch(oracle_mod, ora):
    buf, res, row, pos = M.host_fetch(ora, *M.reqs_len_mix())
    tags = np.array([M.P_DST[r % 4] for r in range(M.P_MIX)], np.uint32)
    m = M.model_unpack(buf, res, row, pos, "view", row_tag=tags)
    with oracle_mod.OracleEngine(M.cfg_mix()) as dst:
        _, st = dst.append(m["tag"], m["len"], buf, m["payload_off"])
        assert st["appended"] == m["records"]
        pay = M.payloads_of(m, buf)
        for p in M.P_DST:
            _, r2, b2, _ = dst.fetch([p], [0], [4096])
            assert [b for _, _, b in parse_records(b2[:int(r2["bytes"][0])])] == [x for x, t in zip(pay, m["tag"]) if t == p]


def test_the_scenarios_hold_their_categories(ora):
    # the length mix: all ten lengths, and packed destinations at every residue of 16
    buf, res, row, pos = M.host_fetch(ora, *M.reqs_len_mix())
    m = M.model_unpack(buf, res, row, pos, "packed")
    assert set(m["len"].tolist()) == set(M.LENMIX) == {0, 1, 15, 16, 17, 31, 32, 33, 100, 4097}
    assert set((m["payload_off"] % 16).tolist()) == set(range(16))
    assert set((m["payload_off"][m["len"] > 0] % 16).tolist()) == set(range(16))
    # the partitions: empty, cut by retention, long
    st = [ora.state(p) for p in range(16)]
    assert st[M.P_EMPTY]["log_end_offset"] == 0 and st[M.P_OLD]["log_start_offset"] > 0
    assert st[M.P_LONG]["log_end_offset"] == M.LONG_RECORDS and st[M.P_LONG]["log_start_offset"] == 0
    assert all(st[p]["log_end_offset"] == 2 * len(M.LENMIX) for p in list(range(M.P_MIX)) + [M.P_BAD])
    assert all(st[p]["log_end_offset"] == 0 for p in M.P_DST) and M.budget_row_is_enospc()
    # the row lists
    for n in (1, 255, 256, 257, 513):
        pidx, cons, mx, offs = M.reqs_rows(n)
        assert len(pidx) == n and (mx[:4].tolist() == [0, 1, 2, 3][:n]) and int(offs.max()) + 3 <= 2 * len(M.LENMIX)
    pidx, cons, mx, offs = M.reqs_shapes()
    assert sorted(mx.tolist()) == [1, 1, 20, 63, 64, 65, 1000] and all(int(o) + int(k) <= M.LONG_RECORDS for o, k, p in zip(offs, mx, pidx) if p == M.P_LONG)
    pidx, cons, mx, offs, bud = M.reqs_non_owning()
    assert pidx[0] == pidx[-1] == M.P_EMPTY and int(offs[2]) < st[M.P_OLD]["log_start_offset"]
    assert int(offs[8]) == st[5]["log_end_offset"] and bud[4] == 16 and pidx[6] == M.P_BAD


def test_the_structure_checks_name_the_lowest_failing_row():
    img = np.zeros(96, np.uint8)
    img[8], img[40], img[72] = 5, 16, 0  # three images of 32 bytes: len 5, len 16, and len 0 (which needs only 16: a mismatch)
    res = M.res_rows([(0, 0, 0, 0, 0), (0, 0, 2, 64, 0), (0, 64, 0, 32, A.RMQ_ENOSPC), (0, 64, 1, 32, 0)])
    row, pos = np.array([0, 0, 3, 3, 5], np.uint64), np.array([0, 32, 64, 0, 32], np.uint64)
    m = M.model_unpack(img, res, row, pos, "packed")
    assert m["status"] == A.RMQ_OK and m["records"] == 3 and list(m["len"]) == [5, 16, 0] and m["mismatched"] == 1
    assert list(m["rec_first"]) == [0, 0, 2, 2, 3] and list(m["tag"]) == [1, 1, 3]

    def bad(**kw):
        a = dict(res=res.copy(), row=row.copy(), pos=pos.copy(), buf_bytes=96, rec_words=5)
        a.update(kw)
        return M.first_bad_row(a["res"], a["row"], a["pos"], a["buf_bytes"], a["rec_words"])

    assert bad() is None
    p = pos.copy(); p[1] = 64
    assert bad(pos=p) == 1          # not increasing by 16
    p = pos.copy(); p[1] = 24
    assert bad(pos=p) == 1          # no multiple of 16
    p = pos.copy(); p[3] = 16
    assert bad(pos=p) == 3          # does not start at 0
    p = pos.copy(); p[4] = 16
    assert bad(pos=p) == 3          # does not end at bytes
    assert bad(rec_words=4) == 3    # rec_row[n] above rec_words
    assert bad(buf_bytes=95) == 3   # out_pos + bytes past buf_bytes
    w = row.copy(); w[2] = 2
    assert bad(row=w) == 1          # the word count is not count + 1
    w = row.copy(); w[1] = 1
    assert bad(row=w) == 0          # a non-owning row with words
    r2 = res.copy(); r2["out_pos"][3] = 72
    assert bad(res=r2) == 3         # out_pos no multiple of 16
