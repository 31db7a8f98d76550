"""RMQ_FETCH_FILL without a GPU: the header's new `mem` bit against the Python mirror, distinct from
the other bits of `mem`, added without a version bump or a struct change, and the message of the
status a filling fetch answers per row."""
import inspect
import os
import subprocess

import pytest

from ripplemq_amd import _abi as A
from ripplemq_amd.engine import FETCH_RES_DTYPE, Engine

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(A.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return A.load()


def test_header_defines_the_flag(tmp_path):
    exe = tmp_path / "abi_layout_fill"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), os.path.join(HERE, "abi_layout_fill.c")], check=True)
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["RMQ_FETCH_FILL"] == A.RMQ_FETCH_FILL == 0x400
    with open(os.path.join(HERE, "..", "include", "ripplemq_engine.h")) as f:
        assert "#define RMQ_FETCH_FILL 0x400u\n" in f.read()
    bits = [got["RMQ_FETCH_FILL"], got["RMQ_FETCH_PINNED_ROWS"], got["RMQ_FETCH_DEVICE_ROWS"]]
    assert bits == [A.RMQ_FETCH_FILL, A.RMQ_FETCH_PINNED_ROWS, A.RMQ_FETCH_DEVICE_ROWS]
    assert all(b & (b - 1) == 0 for b in bits) and len(set(bits)) == 3
    # ... and clear of the memory kinds the bits are ORed to
    assert all(b > max(got["RMQ_MEM_HOST"], got["RMQ_MEM_DEVICE"], got["RMQ_MEM_PINNED"]) for b in bits)
    assert got["RMQ_PENDING"] == A.RMQ_PENDING == 1 and got["RMQ_ENOSPC"] == A.RMQ_ENOSPC
    assert got["RMQ_ABI_VERSION"] == A.RMQ_ABI_VERSION == 11  # no version bump
    assert got["sizeof_rmq_fetch_res"] == FETCH_RES_DTYPE.itemsize == 32  # no struct moves


def test_pending_has_a_message(lib):
    msg = lib.rmq_strerror(A.RMQ_PENDING)
    assert msg and msg != lib.rmq_strerror(-1000)  # (not the unknown-status text)
    assert A.STATUS_NAMES[A.RMQ_PENDING] == "RMQ_PENDING"


def test_python_entry_points_take_fill():
    for f in (Engine.fetch, Engine.fetch_device, Engine.fetch_async):
        p = inspect.signature(f).parameters["fill"]
        assert p.default is False
