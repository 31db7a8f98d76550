"""bench.py's command line: a plain run times --steps appends and prints the line without the side
legs (those sit behind --full); --dump-outputs writes the last timed step's outputs, the same files
for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
FILES = ("offsets", "append_stats", "partition_states", "ring_sample_partitions", "ring_sample")


def _bench(*argv):
    p = subprocess.run([sys.executable, BENCH, *argv], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return p.stdout


def test_options_listed():
    text = _bench("--help")
    assert "--full" in text and "--dump-outputs" in text


@pytest.mark.gpu
def test_plain_run_line_and_outputs(tmp_path):
    steps, warmup, records, parts = 6, 2, 65536, 256  # config A: 65536 records round-robin over 256 partitions
    lines = []
    for d in ("a", "b"):
        out = _bench("--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--config", "A", "--pool", "4",
                     "--dump-outputs", str(tmp_path / d))
        lines.append(json.loads(out.strip().splitlines()[-1]))
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == steps and line["warmup"] == warmup
    # value = records of the timed steps / their time; ms_per_step = that time / steps
    assert line["value"] * line["ms_per_step"] == pytest.approx(records * 1e3, rel=1e-9)
    assert line["cpu_baseline"] is None
    assert not {"host_path", "fetch", "mixed", "tier"} & set(line)

    a = {f: np.load(tmp_path / "a" / f"{f}.npy") for f in FILES}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(f"{f}.npy" for f in FILES)
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for f in FILES:  # seeded inputs: the second run computed the same
        assert np.array_equal(a[f], np.load(tmp_path / "b" / f"{f}.npy")), f
    # the last of warmup + steps batches: each partition's records follow those of the batches before
    per = records // parts
    off = a["offsets"]
    assert off.shape == (records,) and off.min() == (warmup + steps - 1) * per and off.max() == (warmup + steps) * per - 1
    assert a["append_stats"][:2].tolist() == [records, records]  # records, appended
    st = a["partition_states"]
    assert st.shape[0] == parts and np.all(st[:, 0] == (warmup + steps) * per)  # log_end_offset
    assert a["ring_sample"].shape[:2] == (len(a["ring_sample_partitions"]), 3) and a["ring_sample"].any()
