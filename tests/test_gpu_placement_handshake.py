"""The placement handshake between ranks (replication.cpp, FORMAT.md §9): placements whose out and in
lists disagree are refused with RMQ_EINVAL on every rank, and a consistent one is accepted afterwards
and replicates.

Its own two-rank LocalHub and fresh engines (a refused placement does change roles), driven with the
collective helper of test_gpu_control_args. The cases run in order with no append in between; after
each refusal both ranks must still be in lock-step, which the next collective call shows.
"""
import numpy as np
import pytest

from ripplemq_amd.engine import Engine, LocalHub
from test_gpu_control_args import EINVAL, HUB_KEYS, HUB_RANKS, OK, SLOTS, P, _cfg, collective, place

pytestmark = pytest.mark.gpu


def test_refused_placements_then_an_accepted_one_replicates():
    hub, engs = LocalHub(2), [Engine(_cfg(r)) for r in range(2)]

    def placed(rows_of, keys_of):
        rcs = [None, None]

        def fn(r):
            rcs[r] = place(engs[r], range(P), rows_of(r), SLOTS, keys_of(r))

        collective(engs, fn)
        return rcs

    try:
        collective(engs, lambda r: engs[r].attach_local(hub))
        # 1. rank 1 knows partition 0 (led by rank 0, both followers on rank 1) by another key: the
        #    counts agree, the key sums do not
        other = HUB_KEYS.copy()
        other[0] += 1
        assert placed(lambda r: HUB_RANKS, lambda r: other if r else HUB_KEYS) == [EINVAL, EINVAL]
        # 2. rank 1's row of partition 0 gives it one replica fewer than rank 0 sends to
        fewer = HUB_RANKS.copy()
        fewer[0] = [0, 1, 0]
        assert placed(lambda r: fewer if r else HUB_RANKS, lambda r: HUB_KEYS) == [EINVAL, EINVAL]
        # 3. both name rank 2, which the world of two does not have
        beyond = HUB_RANKS.copy()
        beyond[3] = [1, 1, 2]
        assert placed(lambda r: beyond, lambda r: HUB_KEYS) == [EINVAL, EINVAL]
        # 4. the consistent placement; rank 0 starts a term on the partitions it leads (0 by slot 0,
        #    1 by slot 1) and appends a dozen records to them, rank 1 an empty batch (rounds are collective)
        assert placed(lambda r: HUB_RANKS, lambda r: HUB_KEYS) == [OK, OK]
        lens = 5 + np.arange(12, dtype=np.uint32)
        payload = (np.arange(int(lens.sum())) % 251).astype(np.uint8)

        def produce(r):
            e = engs[r]
            if r == 0:
                for p in (0, 1):
                    e.become_leader(p, e.state(p)["term"] + 1)
                e.append_async(np.arange(12) % 2, lens, payload)
            else:
                e.append_async(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
            e.sync()

        collective(engs, produce)
        for p in (0, 1):
            lead, follow = engs[0].state(p), engs[1].state(p)
            assert lead["is_leader"] == 1 and follow["is_leader"] == 0
            assert lead["log_end_offset"] == follow["log_end_offset"] == 6 == lead["commit"], (p, lead, follow)
            ring = engs[0].read_segment(int(SLOTS[p]), p)
            assert ring.any()
            for s in np.flatnonzero(HUB_RANKS[p] == 1):
                assert np.array_equal(engs[1].read_segment(int(s), p), ring), (p, s)
        stats = [e.replication_stats() for e in engs]
        # rank 0 sends partitions 0 and 1 to two slots each and holds two slots of partition 2
        assert [(s["out_entries"], s["in_entries"]) for s in stats] == [(4, 2), (2, 4)], stats
        assert stats[1]["records_ingested"] == 24 and stats[1]["refused_crc"] == stats[1]["refused_log"] == 0, stats
    finally:
        for e in engs:
            e.close()
        hub.close()
