"""Times the state read-backs of the tree given as argv[1]: 1,000 single rmq_get_partition_state calls on an
idle engine of 256 partitions, and 200 bulk rmq_get_partition_states of 4,096 partitions. One JSON line."""
import json
import statistics
import sys
import time

sys.path.insert(0, sys.argv[1])
import numpy as np  # noqa: E402

from ripplemq_amd.engine import Engine, EngineConfig  # noqa: E402


def per_call(fn, calls):
    ts = []
    for k in range(calls):
        t0 = time.perf_counter()
        fn(k)
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e6, sum(ts) / calls * 1e6


out = {}
with Engine(EngineConfig(num_partitions=256, replication_factor=3, segment_bytes=1 << 16, index_interval=1024)) as e:
    lens = np.full(1024, 100, np.uint32)
    e.append(np.arange(1024) % 256, lens, np.zeros(int(lens.sum()), np.uint8))
    e.sync()
    for k in range(50):
        e.state(k)
    out["single_p256_median_us"], out["single_p256_mean_us"] = per_call(lambda k: e.state(k % 256), 1000)
with Engine(EngineConfig(num_partitions=4096, replication_factor=3, segment_bytes=1 << 16, index_interval=1024)) as e:
    for k in range(20):
        e.states()
    out["bulk_p4096_median_us"], out["bulk_p4096_mean_us"] = per_call(lambda k: e.states(), 200)
print(json.dumps(out))
