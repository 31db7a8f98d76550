"""rmq_fetch_table without a GPU: the two exports exist with the header's prototypes, added without a
version bump or a struct change; with null table arguments the call is rmq_fetch_at (here: what both
answer to a null engine); the table's own argument checks come before anything touches a device; and
the Python entry points take the table."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

from ripplemq_amd import _abi as A
from ripplemq_amd.engine import FETCH_RES_DTYPE, RESTORE_ITEM_DTYPE, Engine

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(A.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return A.load()


def test_header_declares_the_two_functions(tmp_path):
    exe = tmp_path / "abi_layout_table"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), os.path.join(HERE, "abi_layout_table.c")],
                   check=True)  # (a prototype that differs from the documented argument list does not compile)
    got = {k: int(v) for k, v in (line.rsplit(" ", 1) for line in subprocess.run(
        [str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())}
    assert got["declared"] == 1
    assert got["RMQ_ABI_VERSION"] == A.RMQ_ABI_VERSION == 11  # no version bump
    assert got["sizeof_rmq_fetch_res"] == FETCH_RES_DTYPE.itemsize == 32  # no struct moves
    assert got["sizeof_rmq_fetch_req"] == 16 and got["sizeof_rmq_restore_item"] == RESTORE_ITEM_DTYPE.itemsize == 64
    assert (got["RMQ_MEM_HOST"], got["RMQ_MEM_DEVICE"]) == (A.RMQ_MEM_HOST, A.RMQ_MEM_DEVICE) == (0, 1)
    assert {"rmq_fetch_table", "rmq_fetch_table_async"} <= set(A.header_symbols())


def test_exports_exist_and_null_arguments_answer_as_fetch_at(lib):
    assert hasattr(lib, "rmq_fetch_table") and hasattr(lib, "rmq_fetch_table_async")
    assert A._SIGS["rmq_fetch_table"][1][:9] == A._SIGS["rmq_fetch_at"][1][:9]  # everything rmq_fetch_at takes, first
    used = C.c_uint64(7)
    at = lib.rmq_fetch_at(None, None, None, None, 0, A.RMQ_MEM_HOST, None, 0, None, C.byref(used))
    assert (at, used.value) == (A.RMQ_EINVAL, 0)
    used = C.c_uint64(7)
    tb = lib.rmq_fetch_table(None, None, None, None, 0, A.RMQ_MEM_HOST, None, 0, None, None, None, 0, C.byref(used))
    assert (tb, used.value) == (at, 0)
    t = C.c_uint64(0)
    assert lib.rmq_fetch_table_async(None, None, None, None, 0, A.RMQ_MEM_HOST, None, 0, None, None, None, 0,
                                     C.byref(t)) == lib.rmq_fetch_at_async(None, None, None, None, 0, A.RMQ_MEM_HOST,
                                                                           None, 0, None, C.byref(t)) == A.RMQ_EINVAL


def test_the_walk_program_builds_and_passes(tmp_path):
    """tools/fetch_table_walk_main.cpp (the walk's step, scalar and lane by lane, over damaged runs)
    as an ordinary build; its header comment gives the sanitizer build."""
    exe = tmp_path / "fetch_table_walk"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe),
                    os.path.join(HERE, "..", "tools", "fetch_table_walk_main.cpp")], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert out.startswith("fetch_table_walk: ok (3000 runs")


def test_python_entry_points_take_a_table():
    for f in (Engine.fetch, Engine.fetch_device, Engine.fetch_async):
        assert inspect.signature(f).parameters["table"].default is None
    from ripplemq_amd import table_records  # noqa: F401
    from ripplemq_amd.state_machine import PartitionBroker

    assert inspect.signature(PartitionBroker.__init__).parameters["record_table"].default is False
