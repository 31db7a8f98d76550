"""rmq_reindex's ABI without a GPU: rmq_reindex_res's layout against the ctypes and numpy mirrors,
the two flags, the argument checks that need no device, and the ABI version, which the additions
leave at 11."""
import ctypes as C
import os
import subprocess

import pytest

from ripplemq_amd import _abi as A

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(A.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return A.load()


def test_reindex_res_layout_and_constants(tmp_path):
    from ripplemq_amd.engine import REINDEX_RES_DTYPE

    exe = tmp_path / "abi_layout_reindex"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), os.path.join(HERE, "abi_layout_reindex.c")], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                               check=True).stdout.splitlines())
    assert C.sizeof(A.RmqReindexRes) == int(got.pop("rmq_reindex_res")) == REINDEX_RES_DTYPE.itemsize == 48
    fields = [k for k in got if "." in k]
    assert [k.split(".")[1] for k in fields] == [f for f, _ in A.RmqReindexRes._fields_] == list(REINDEX_RES_DTYPE.names)
    for k in fields:
        f = k.split(".")[1]
        assert getattr(A.RmqReindexRes, f).offset == int(got[k]) == REINDEX_RES_DTYPE.fields[f][1], k
    assert int(got["RMQ_ABI_VERSION"]) == A.RMQ_ABI_VERSION == 11
    assert int(got["RMQ_REINDEX_DRY_RUN"]) == A.RMQ_REINDEX_DRY_RUN == 1
    assert int(got["RMQ_REINDEX_ALL"]) == A.RMQ_REINDEX_ALL == 2


def test_null_engine_is_invalid_and_the_version_stays(lib):
    res = A.RmqReindexRes()
    assert lib.rmq_reindex(None, 0, 1, 0, C.byref(res)) == A.RMQ_EINVAL
    assert lib.rmq_reindex(None, 0, 0, A.RMQ_REINDEX_DRY_RUN | A.RMQ_REINDEX_ALL, None) == A.RMQ_EINVAL
    assert lib.rmq_fault_flip_index(None, 0, 0, 0, 1) == A.RMQ_EINVAL
    assert lib.rmq_abi_version() == 11
    for name in ("rmq_reindex", "rmq_fault_flip_index"):
        assert name in A.header_symbols() and name in A._SIGS
