"""rmq_restore's ABI without a GPU: the layouts of rmq_restore_item and rmq_restore_res against the
ctypes and numpy mirrors, the flag, the argument checks that need no device, and the ABI version,
which the addition leaves at 11."""
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


def test_restore_layouts_and_constants(tmp_path):
    from ripplemq_amd.engine import RESTORE_ITEM_DTYPE, RESTORE_RES_DTYPE

    exe = tmp_path / "abi_layout_restore"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), os.path.join(HERE, "abi_layout_restore.c")], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                               check=True).stdout.splitlines())
    assert C.sizeof(A.RmqRestoreItem) == int(got.pop("rmq_restore_item")) == RESTORE_ITEM_DTYPE.itemsize == 64
    assert C.sizeof(A.RmqRestoreRes) == int(got.pop("rmq_restore_res")) == RESTORE_RES_DTYPE.itemsize == 32
    for name, ct, dt in (("rmq_restore_item", A.RmqRestoreItem, RESTORE_ITEM_DTYPE),
                         ("rmq_restore_res", A.RmqRestoreRes, RESTORE_RES_DTYPE)):
        fields = [k for k in got if k.startswith(name + ".")]
        assert [k.split(".")[1] for k in fields] == [f for f, _ in ct._fields_] == list(dt.names)
        for k in fields:
            f = k.split(".")[1]
            assert getattr(ct, f).offset == int(got[k]) == dt.fields[f][1], k
    assert int(got["RMQ_ABI_VERSION"]) == A.RMQ_ABI_VERSION == 11
    assert int(got["RMQ_RESTORE_DRY_RUN"]) == A.RMQ_RESTORE_DRY_RUN == 1


def test_null_engine_is_invalid_and_the_version_stays(lib):
    item, res = A.RmqRestoreItem(), A.RmqRestoreRes()
    assert lib.rmq_restore(None, 1, C.byref(item), A.RMQ_MEM_HOST, None, 0, None, 0, 0, C.byref(res)) == A.RMQ_EINVAL
    assert lib.rmq_restore(None, 0, None, A.RMQ_MEM_HOST, None, 0, None, 0, A.RMQ_RESTORE_DRY_RUN, None) == A.RMQ_EINVAL
    assert lib.rmq_abi_version() == 11
    assert "rmq_restore" in A.header_symbols() and "rmq_restore" in A._SIGS
    assert A.header_symbols() == sorted(A._SIGS)
