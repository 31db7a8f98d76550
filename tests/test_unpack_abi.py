"""rmq_unpack's ABI without a GPU: the layout of rmq_unpack_args and rmq_unpack_res against the ctypes
and numpy mirrors, the sizes and the ABI version the addition leaves alone, the export, the argument
checks (they answer before the engine or a device is touched), the stand-alone checker and the
Python entry points."""
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


def test_layouts_and_what_stays(tmp_path):
    from ripplemq_amd.engine import UNPACK_ARGS_DTYPE, UNPACK_RES_DTYPE

    exe = tmp_path / "abi_layout_unpack"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), os.path.join(HERE, "abi_layout_unpack.c")],
                   check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                               check=True).stdout.splitlines())
    want_args = dict(buf=0, buf_bytes=8, rows=16, rec_row=24, rec_pos=32, rec_words=40, row_tag=48, rec_first=56,
                     offset=64, len=72, payload_off=80, tag=88, rec_cap=96, payload=104, payload_cap=112, n=120,
                     stride=124, mem=128, flags=132)
    want_res = dict(records=0, payload_bytes=8, mismatched=16, truncated=24, bad_row=32, status=40, reserved=44)
    for name, struct, dtype, size, want in (("rmq_unpack_args", A.RmqUnpackArgs, UNPACK_ARGS_DTYPE, 136, want_args),
                                            ("rmq_unpack_res", A.RmqUnpackRes, UNPACK_RES_DTYPE, 48, want_res)):
        assert C.sizeof(struct) == int(got.pop(name)) == dtype.itemsize == size
        fields = [k for k in got if k.startswith(name + ".")]
        assert [k.split(".")[1] for k in fields] == [f for f, _ in struct._fields_] == list(dtype.names) == list(want)
        for k in fields:
            f = k.split(".")[1]
            assert getattr(struct, f).offset == int(got[k]) == dtype.fields[f][1] == want[f], k
    assert int(got["RMQ_ABI_VERSION"]) == A.RMQ_ABI_VERSION == 11
    assert int(got["rmq_fetch_req"]) == C.sizeof(A.RmqFetchReq) == 16
    assert int(got["rmq_fetch_res"]) == C.sizeof(A.RmqFetchRes) == 32
    assert int(got["rmq_lag_res"]) == C.sizeof(A.RmqLagRes) == 64
    assert int(got["rmq_batch"]) == C.sizeof(A.RmqBatch) == 48
    assert int(got["rmq_restore_item"]) == 64


def test_export_and_signature(lib):
    assert hasattr(lib, "rmq_unpack") and lib.rmq_abi_version() == 11
    assert "rmq_unpack" in A.header_symbols() and "rmq_unpack" in A._SIGS
    assert A.header_symbols() == sorted(A._SIGS)
    nm = subprocess.run(["nm", "-D", "--defined-only", A.LIB_PATH], capture_output=True, text=True).stdout
    assert " T rmq_unpack\n" in nm


def _args(**kw):
    d = 1 << 20  # addresses that are never dereferenced
    base = dict(buf=d, buf_bytes=4096, rows=d + 4096, rec_row=2 * d, rec_pos=3 * d, rec_words=64, row_tag=None,
                rec_first=4 * d, offset=5 * d, len=6 * d, payload_off=7 * d, tag=8 * d, rec_cap=16, payload=9 * d + 3,
                payload_cap=4096, n=4, stride=0, mem=A.RMQ_MEM_DEVICE | A.RMQ_FETCH_DEVICE_ROWS, flags=0)
    base.update(kw)
    return A.RmqUnpackArgs(**base)


def test_argument_checks_answer_before_anything_is_touched(lib):
    """Every refused call returns from the checks alone: the engine handle here is a block of zero
    bytes that is no engine (no device, no stream), no array is read or written, and `out` stays as
    it was."""
    fake = (C.c_uint8 * 65536)()
    e = C.addressof(fake)
    out = np.full(48, 0xEE, np.uint8)
    p_out = out.ctypes.data
    EINVAL = A.RMQ_EINVAL

    def call(eng, a, o=p_out):
        return lib.rmq_unpack(eng, None if a is None else C.byref(a), o)

    # a null engine, null args, null out
    assert call(None, _args()) == EINVAL and call(e, None) == EINVAL and call(e, _args(), None) == EINVAL
    assert call(None, _args(n=0)) == EINVAL
    # mem: device output only, host rows or device rows
    for mem in (A.RMQ_MEM_HOST, A.RMQ_MEM_PINNED, 3, A.RMQ_MEM_HOST | A.RMQ_FETCH_DEVICE_ROWS,
                A.RMQ_MEM_DEVICE | A.RMQ_FETCH_FILL, A.RMQ_MEM_DEVICE | A.RMQ_FETCH_PINNED_ROWS, 0x80000001):
        assert call(e, _args(mem=mem)) == EINVAL, mem
    # flags
    for fl in (1, 2, 0x80000000):
        assert call(e, _args(flags=fl)) == EINVAL, fl
    # misaligned pointers (the payload may sit anywhere; host rows too)
    d = 1 << 20
    for k, v in (("buf", d + 8), ("rows", d + 8), ("rec_row", d + 4), ("rec_pos", d + 4), ("row_tag", d + 2),
                 ("rec_first", d + 4), ("offset", d + 4), ("len", d + 2), ("payload_off", d + 4), ("tag", d + 1)):
        assert call(e, _args(**{k: v})) == EINVAL, k
    # null required pointers with n != 0
    for k in ("rows", "rec_row", "rec_first", "rec_pos", "buf", "len", "payload_off"):
        assert call(e, _args(**{k: None})) == EINVAL, k
    # a mode mismatch: view mode with a stride or a payload capacity
    assert call(e, _args(payload=None, payload_cap=0, stride=16)) == EINVAL
    assert call(e, _args(payload=None, payload_cap=4096)) == EINVAL
    assert call(e, _args(payload=None, payload_cap=0, stride=0, n=0, mem=7)) == EINVAL
    assert (out == 0xEE).all()
    # n == 0 without rec_first: RMQ_OK, R = 0, nothing but `out` is touched
    for a in (_args(n=0, rec_first=None), _args(n=0, rec_first=None, rows=None, rec_row=None, rec_pos=None, buf=None,
                                                 len=None, payload_off=None, mem=A.RMQ_MEM_DEVICE)):
        out[:] = 0xEE
        assert call(e, a) == A.RMQ_OK
        res = A.RmqUnpackRes.from_buffer_copy(out.tobytes())
        assert (res.records, res.payload_bytes, res.mismatched, res.truncated, res.status, res.reserved) == (0,) * 6
        assert res.bad_row == A.RMQ_OFFSET_NONE
    assert not any(fake)


def test_checker_builds_and_passes(tmp_path):
    exe = tmp_path / "unpack_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(REPO, "tools", "unpack_check_main.cpp")],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert out.startswith("unpack_check: ok ("), out


def test_python_entry_points_exist():
    import inspect

    from ripplemq_amd.engine import UNPACK_RES_DTYPE, Engine
    from ripplemq_amd.state_machine import PartitionBroker

    assert UNPACK_RES_DTYPE.itemsize == 48
    for name in ("unpack_device", "fetch_columns"):
        assert callable(getattr(Engine, name)), name
    assert inspect.signature(PartitionBroker.__init__).parameters["columns"].default is False
    p = inspect.signature(Engine.fetch_columns).parameters
    assert p["mode"].default == "packed" and p["row_tag"].default is None
