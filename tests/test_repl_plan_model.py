"""The replication plan without a GPU: the stand-alone checker of ripplemq_amd/csrc/repl_plan.hpp (lists
from a placement, buffer bounds, a round's layout) builds and passes, and the catch-up reserve it
computes is the oracle's."""
import os
import subprocess

import pytest

from ripplemq_amd.engine import EngineConfig

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def checker_output(tmp_path_factory):
    exe = tmp_path_factory.mktemp("repl_plan") / "repl_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-o", str(exe), os.path.join(REPO, "tools", "repl_plan_main.cpp")], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_plan_checker_builds_and_passes(checker_output):
    assert checker_output[-1].startswith("repl_plan: ok ("), checker_output


def test_reserve_is_the_oracles(checker_output):
    from oracle.oracle import OracleEngine

    rows = [dict(zip(w[1::2], map(int, w[2::2]))) for w in (line.split() for line in checker_output) if w[0] == "bounds"]
    assert len(rows) == 2
    for r, depth in zip(rows, ({}, {"pipeline_depth": 8})):  # the default depth, then 8
        cfg = EngineConfig(num_partitions=4, replication_factor=3, max_batch_records=r["max_batch_records"],
                           max_batch_bytes=r["max_batch_bytes"], **depth)
        assert r["group_max"] == cfg.pipeline_depth
        with OracleEngine(cfg) as ora:
            assert r["reserve"] == ora.catchup_reserve() == cfg.pipeline_depth * (39 * cfg.max_batch_records + cfg.max_batch_bytes)
