"""ABI 11 without a GPU: rmq_scrub_res's layout against the ctypes and numpy mirrors, the new status
code and its message, the new constants, and the argument checks that need no device."""
import ctypes as C
import os
import subprocess

import pytest

from ripplemq_amd import _abi as A
from ripplemq_amd.engine import SCRUB_RES_DTYPE

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(A.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return A.load()


def test_scrub_res_layout_and_constants(tmp_path):
    exe = tmp_path / "abi_layout_scrub"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), os.path.join(HERE, "abi_layout_scrub.c")], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                               check=True).stdout.splitlines())
    assert C.sizeof(A.RmqScrubRes) == int(got.pop("rmq_scrub_res")) == SCRUB_RES_DTYPE.itemsize == 40
    fields = [k for k in got if "." in k]
    assert [k.split(".")[1] for k in fields] == [f for f, _ in A.RmqScrubRes._fields_] == list(SCRUB_RES_DTYPE.names)
    for k in fields:
        f = k.split(".")[1]
        assert getattr(A.RmqScrubRes, f).offset == int(got[k]) == SCRUB_RES_DTYPE.fields[f][1], k
    assert int(got["RMQ_ABI_VERSION"]) == A.RMQ_ABI_VERSION == 11
    assert int(got["RMQ_ECORRUPT"]) == A.RMQ_ECORRUPT == -10
    assert int(got["RMQ_FETCH_VERIFY"]) == A.RMQ_FETCH_VERIFY == 0x20
    assert (int(got["RMQ_SCRUB_BAD_CRC"]), int(got["RMQ_SCRUB_BAD_CHAIN"])) == (A.RMQ_SCRUB_BAD_CRC, A.RMQ_SCRUB_BAD_CHAIN) == (1, 2)
    # the flags of a fetch request stay distinct bits, apart from the row-kind bits of `mem`
    assert len({A.RMQ_FETCH_COMMIT, A.RMQ_FETCH_REPLICA, A.RMQ_FETCH_VERIFY}) == 3
    assert A.RMQ_FETCH_COMMIT & A.RMQ_FETCH_VERIFY == 0 and A.RMQ_FETCH_REPLICA & A.RMQ_FETCH_VERIFY == 0


def test_abi_version_and_corrupt_message(lib):
    assert lib.rmq_abi_version() == 11
    msg = lib.rmq_strerror(A.RMQ_ECORRUPT)
    assert msg == b"record checksum or log structure is corrupt"
    assert msg != lib.rmq_strerror(-1000)  # (not the unknown-status text)
    assert A.STATUS_NAMES[A.RMQ_ECORRUPT] == "RMQ_ECORRUPT"


def test_null_engine_is_invalid(lib):
    res = A.RmqScrubRes()
    assert lib.rmq_scrub(None, 0, 1, C.byref(res)) == A.RMQ_EINVAL
    assert lib.rmq_scrub(None, 0, 0, None) == A.RMQ_EINVAL
    assert lib.rmq_fault_flip_ring(None, 0, 0, 0, 0x5A) == A.RMQ_EINVAL
