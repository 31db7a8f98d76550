"""rmq_lag's ABI without a GPU: the layout of rmq_lag_res against the ctypes and numpy mirrors, the
sizes and the ABI version the addition leaves alone, the export, the argument checks (they answer
before the engine or a device is touched), the stand-alone row checker and the Python entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from ripplemq_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(A.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return A.load()


def test_lag_res_layout_and_what_stays(tmp_path):
    from ripplemq_amd.engine import LAG_RES_DTYPE

    exe = tmp_path / "abi_layout_lag"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), os.path.join(HERE, "abi_layout_lag.c")],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                               check=True).stdout.splitlines())
    assert C.sizeof(A.RmqLagRes) == int(got.pop("rmq_lag_res")) == LAG_RES_DTYPE.itemsize == 64
    fields = [k for k in got if k.startswith("rmq_lag_res.")]
    assert [k.split(".")[1] for k in fields] == [f for f, _ in A.RmqLagRes._fields_] == list(LAG_RES_DTYPE.names)
    want = dict(start_offset=0, records=8, bytes=16, evicted=24, start_pos=32, end_pos=40, headroom=48, status=56,
                reserved=60)
    for k in fields:
        f = k.split(".")[1]
        assert getattr(A.RmqLagRes, f).offset == int(got[k]) == LAG_RES_DTYPE.fields[f][1] == want[f], k
    assert int(got["RMQ_ABI_VERSION"]) == A.RMQ_ABI_VERSION == 11
    assert int(got["rmq_fetch_req"]) == C.sizeof(A.RmqFetchReq) == 16
    assert int(got["rmq_fetch_res"]) == C.sizeof(A.RmqFetchRes) == 32


def test_export_and_signature(lib):
    assert hasattr(lib, "rmq_lag") and lib.rmq_abi_version() == 11
    assert "rmq_lag" in A.header_symbols() and "rmq_lag" in A._SIGS
    assert A.header_symbols() == sorted(A._SIGS)
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True).stdout
    assert " T rmq_lag\n" in nm


def test_argument_checks_answer_before_anything_is_touched(lib):
    """Every refused call returns from the checks alone: the engine handle here is a block of zero
    bytes that is no engine (no device, no stream), and the rows are never read or written."""
    req = np.zeros((4, 4), np.uint32)
    res = np.full(4, 0xEE, np.uint8).repeat(64).view(np.uint8)
    offs = np.zeros(4, np.uint64)
    fake = (C.c_uint8 * 65536)()
    e = C.addressof(fake)
    p_req, p_res, p_at = req.ctypes.data, res.ctypes.data, offs.ctypes.data
    EINVAL = A.RMQ_EINVAL
    # a null engine, whatever else is passed
    assert lib.rmq_lag(None, p_req, None, 4, A.RMQ_MEM_HOST, p_res) == EINVAL
    assert lib.rmq_lag(None, None, None, 0, A.RMQ_MEM_HOST, None) == EINVAL
    # null rows with n != 0
    assert lib.rmq_lag(e, None, None, 4, A.RMQ_MEM_HOST, p_res) == EINVAL
    assert lib.rmq_lag(e, p_req, None, 4, A.RMQ_MEM_HOST, None) == EINVAL
    assert lib.rmq_lag(e, None, p_at, 1, A.RMQ_MEM_DEVICE, None) == EINVAL
    # an unknown mem, and every RMQ_FETCH_* bit of the fetch calls' mem word
    for mem in (A.RMQ_MEM_PINNED, 3, 7, A.RMQ_MEM_HOST | A.RMQ_FETCH_FILL, A.RMQ_MEM_DEVICE | A.RMQ_FETCH_FILL,
                A.RMQ_MEM_DEVICE | A.RMQ_FETCH_DEVICE_ROWS, A.RMQ_MEM_HOST | A.RMQ_FETCH_PINNED_ROWS, 0x80000000):
        assert lib.rmq_lag(e, p_req, None, 4, mem, p_res) == EINVAL, mem
    # misaligned device pointers (these addresses are never dereferenced)
    d = 1 << 20
    for rq, at, rs in ((d + 8, None, d), (d, None, d + 8), (d + 4, None, d), (d, d + 4, d), (d, d + 2, d), (d + 1, d, d + 1)):
        assert lib.rmq_lag(e, C.c_void_p(rq), None if at is None else C.c_void_p(at), 4, A.RMQ_MEM_DEVICE,
                           C.c_void_p(rs)) == EINVAL, (rq, at, rs)
    # an unknown flag bit in a host row
    for bit in (4, 8, 16, 0x40, 0x80000000):
        bad = req.copy()
        bad[2, 3] = A.RMQ_FETCH_REPLICA | bit
        assert lib.rmq_lag(e, bad.ctypes.data, None, 4, A.RMQ_MEM_HOST, p_res) == EINVAL, bit
    # n == 0 is RMQ_OK and touches nothing
    assert lib.rmq_lag(e, None, None, 0, A.RMQ_MEM_HOST, None) == A.RMQ_OK
    assert lib.rmq_lag(e, p_req, p_at, 0, A.RMQ_MEM_DEVICE, p_res) == A.RMQ_OK
    assert (res == 0xEE).all() and not any(fake) and not req.any()


def test_row_checker_builds_and_passes(tmp_path):
    exe = tmp_path / "lag_row"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(REPO, "tools", "lag_row_main.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert out.startswith("lag_row: ok ("), out


def test_python_entry_points_exist():
    from ripplemq_amd.engine import LAG_RES_DTYPE, Engine
    from ripplemq_amd.state_machine import PartitionBroker
    from ripplemq_amd.tier import DurableLog

    assert LAG_RES_DTYPE.itemsize == 64
    for owner, name in ((Engine, "lag"), (Engine, "lag_device"), (PartitionBroker, "consumer_lag"), (DurableLog, "backlog")):
        assert callable(getattr(owner, name)), name
