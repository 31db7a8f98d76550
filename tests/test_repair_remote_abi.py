"""rmq_repair_remote's ABI without a GPU: rmq_repair_remote_res's layout against the ctypes and numpy
mirrors, the exported symbols, the argument checks that need no device, the status messages and the
ABI version, which the additions leave at 11."""
import ctypes as C
import os
import subprocess

import pytest

from ripplemq_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))

FIELDS = ["segments_repaired", "bytes_repaired", "segments_fetched", "bytes_fetched", "segments_unrepaired",
          "bad_offset", "bad_replica", "bad_kind", "replicas", "status"]
OFFSETS = [0, 8, 16, 24, 32, 40, 48, 52, 56, 60]  # the issue's struct: six u64, three u32, one i32
MESSAGES = {  # rmq_strerror before this call existed
    "RMQ_PENDING": b"pending", "RMQ_OK": b"ok", "RMQ_ENOTLEADER": b"Not leader", "RMQ_ENOPART": b"unknown partition",
    "RMQ_EINVAL": b"invalid argument", "RMQ_ENOSPC": b"no space", "RMQ_EDEVICE": b"device error",
    "RMQ_EOFFSET": b"offset out of range", "RMQ_ENOMEM": b"out of memory",
    "RMQ_ESTALE": b"replica lags the committed log", "RMQ_ETERM": b"term already led or voted for another candidate",
    "RMQ_ECORRUPT": b"record checksum or log structure is corrupt",
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(A.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return A.load()


def test_repair_remote_res_layout_and_constants(tmp_path):
    from ripplemq_amd.engine import REPAIR_REMOTE_RES_DTYPE

    exe = tmp_path / "abi_layout_repair_remote"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), os.path.join(HERE, "abi_layout_repair_remote.c")], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                               check=True).stdout.splitlines())
    assert C.sizeof(A.RmqRepairRemoteRes) == int(got.pop("rmq_repair_remote_res")) == REPAIR_REMOTE_RES_DTYPE.itemsize == 64
    fields = [k for k in got if "." in k]
    assert [k.split(".")[1] for k in fields] == [f for f, _ in A.RmqRepairRemoteRes._fields_] == \
        list(REPAIR_REMOTE_RES_DTYPE.names) == FIELDS
    for k, want in zip(fields, OFFSETS):
        f = k.split(".")[1]
        assert getattr(A.RmqRepairRemoteRes, f).offset == int(got[k]) == REPAIR_REMOTE_RES_DTYPE.fields[f][1] == want, k
    assert int(got["RMQ_ABI_VERSION"]) == A.RMQ_ABI_VERSION == 11
    assert int(got["RMQ_REPAIR_DRY_RUN"]) == A.RMQ_REPAIR_DRY_RUN == 1


def test_symbols_null_engine_flags_and_messages(lib):
    for name in ("rmq_repair_remote", "rmq_fault_corrupt_repair"):
        assert hasattr(lib, name) and name in A.header_symbols() and name in A._SIGS
    res = A.RmqRepairRemoteRes()
    served = (C.c_uint64 * 2)(7, 7)
    assert lib.rmq_repair_remote(None, 0, 1, 0, C.byref(res), served) == A.RMQ_EINVAL
    assert lib.rmq_repair_remote(None, 0, 0, A.RMQ_REPAIR_DRY_RUN, None, None) == A.RMQ_EINVAL
    for flags in (2, 3, 0x80000000):  # an unknown flag bit (with an engine: tests/test_gpu_repair_remote.py)
        assert lib.rmq_repair_remote(None, 0, 1, flags, None, None) == A.RMQ_EINVAL
    assert lib.rmq_fault_corrupt_repair(None, 0, 0) == A.RMQ_EINVAL
    assert lib.rmq_abi_version() == 11
    assert {A.STATUS_NAMES[k]: lib.rmq_strerror(k) for k in A.STATUS_NAMES} == MESSAGES
    assert lib.rmq_strerror(-1000) == b"unknown status"
