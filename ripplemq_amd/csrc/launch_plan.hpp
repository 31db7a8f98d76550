// launch_plan.hpp — the knobs rmq_create reads from the environment, and how many workgroups each
// role of one pipeline launch gets: a pure function of the knobs and a dozen integers of the launch.
// Plain C++ with no device header, so that it also builds into a stand-alone program under the
// sanitizers (tools/launch_plan_main.cpp).
#pragma once
#include <algorithm>
#include <cstdint>

namespace rmq {

// Every value rmq_create reads from the environment (once, at create), with its default.
struct Knobs {
  uint32_t trace = 0;      // RMQ_TRACE: print every launch's roles to stderr
  uint32_t debug = 0;      // RMQ_DEBUG (timing experiments only; results are invalid when set)
  uint32_t rank_mode = 0;  // RMQ_RANK: stage 1 by the LDS radix sort (0) or by hash counters (1;
                           // 4.86 vs 5.14 G msgs/s at config B, profiles/r04c_*)
  uint32_t max_ahead = 0;  // RMQ_AHEAD: pipeline launches queued at most (0: unbounded; a bound of
                           // 4 or 8 cost 4-6 % at config B, profiles/r04i_*: bound it in the app)
  uint32_t steal = 0;      // RMQ_STEAL=1: stage-3 workgroups take stage-1 tiles when out of tasks
  uint32_t prio = 1;       // RMQ_PRIO (round 6 default 1; 0 off): stage-1/2 and partition waves at s_setprio 3
                           // (5.20 -> 4.00 G msgs/s: stage 2 and the second half of stage 3 start later)
  // one stage-3 wave per task: the workgroups beyond the resident slots dispatch as stage-1/2
  // workgroups retire (RMQ_WG3_ALL=0: only as many as fit next to them, looping over tasks)
  uint32_t wg3_all = 1;
  uint32_t s1_wgs = 0;    // RMQ_S1_WGS: stage-1 workgroups per launch (0: one per tile; fewer loop over tiles)
  uint32_t s2_wgs = 0;    // RMQ_S2_WGS: cap on stage-2 workgroups (0: one thread group per column)
  uint32_t big_wgs = 0;   // RMQ_BIG_WGS: stage-3 workgroups for records over 1 KB (0: 32 waves per CU)
  uint32_t s3_first = 0;  // RMQ_S3_FIRST=1: stage-3 workgroups first in dispatch order (round 6 default: last, -2.5 %)
  uint32_t s3_lead = 0;   // RMQ_S3_LEAD: stage-3 workgroups before the other roles (0: all of them or none, by s3_first)
  // Split launches (single-GPU kernel, no transport): each pipeline step is two launches of the
  // pipeline kernel that run side by side, the ranking roles (stage 1 of group g, stage 2 of g - 1)
  // on rank_s and the apply roles (stage 3 of g - 2, partition threads, stage 4) on main_s. Rank
  // launch L waits for everything main_s issued before it (apply L - 1 resets the set stage 1 of L
  // reuses); apply launch L waits for rank launch L - 1 (the scans of the group it applies).
  // RMQ_SPLIT=1 (2: the two launches one after the other, timing only); 0 default: one launch per
  // step with every role (the split measured slower: 60 vs 49 us per step). Forced to 0
  // at create by RMQ_STAMPS and RMQ_STEAL (phase stamps and stealing read one launch's roles).
  uint32_t split = 0;
  uint32_t rank_cus = 0;  // RMQ_RANK_CUS=n: rank_s runs on n CUs and main_s on the others
  uint32_t s3_pair = 0;   // RMQ_S3_PAIR=1: stage-3 waves take two tasks each (single-GPU kernel)
  uint32_t s3_roles = 0;  // RMQ_S3_ROLES=k: stage 3 in loader / storer waves, k workgroups per CU (single-GPU kernel)
  uint32_t s3_stage = 1;  // RMQ_S3_STAGE (default 1): stage-3 payload spans by coalesced loads through LDS
  uint32_t s3_xcd = 1;    // RMQ_S3_XCD (default 1): stage-3 tasks in contiguous ranges per XCD
                          //   (blockIdx % 8); round 5: 5.51-5.58 vs 5.43-5.51 G, 3 pairs, r05X8
  uint32_t s1_xcd = 0;    // RMQ_S1_XCD=1: stage-1 tiles in contiguous ranges per XCD
  uint32_t fetch_coalesce = 4;  // RMQ_FETCH_COALESCE: asynchronous fetches launched together (1: none; at most kFetchBatch)
  // RMQ_FETCH_DMA: host request / result rows of a fetch moved by DMA (request rows on copy_s before
  // the kernels, result rows on fetch_out_s after them) instead of read and written in place by
  // the kernels across PCIe: 0 never (default), 1 for rmq_fetch_async, 2 for every fetch. Measured
  // (round 5, tools/exp_dma.sh): the kernels gain 4-11 us but each fetch's copies and cross-stream
  // waits add ~100 us (max = 10 bursts 3.3 -> 1.1 G records/s), so in place stays the default
  uint32_t fetch_dma = 0;
  uint32_t fetch_dma_in = 1;  // RMQ_FETCH_DMA_IN=0: with DMA, the request rows still read in place
  uint32_t verify_wgs = 0;    // RMQ_VERIFY_WGS (at least 1): follower verify grid (0 here: 4 workgroups per CU, set at create)
  uint32_t audit_wgs = 0;     // RMQ_AUDIT_WGS: scrub verify and fetch verify grids at most (0: 8 workgroups per CU)
  uint64_t stamps_at = 100;   // RMQ_STAMPS_AT: the launch whose per-wave phase stamps RMQ_STAMPS=<csv> records
  uint64_t repair_peer_bytes = 64ull << 20;  // RMQ_REPAIR_PEER_BYTES: segment bytes asked of one rank per round (a capacity)
};

// One launch, as far as its grid depends on it.
struct LaunchShape {
  uint32_t P = 0;           // partitions
  uint32_t scan_threads = 0;  // stage 2: kScanLanes threads per group of kScanCols partition columns
  uint32_t cu_count = 0;
  uint32_t threads = 0;     // per workgroup: 512 for the kernel with a transport's outboxes, else 256
  uint32_t wgs_per_cu = 0;  // resident workgroups of that size per CU (pipeline_wgs_per_cu(threads))
  bool transport = false;   // a transport with remote replicas is attached (PipeArgs::outidx)
  bool acks = false;        // followers' acks are due with this launch (PipeArgs::ackin)
  bool repl = false;        // a replication transport is attached at all
  bool s1 = false, s2 = false, s3 = false, s4 = false;  // the stages that have a group
  uint32_t s1_tiles = 0;    // tiles of stage 1's group
  uint32_t s3_tasks = 0;    // tasks of stage 3's group
};

// Workgroups per role and stage 3's variant flags (the fields of the same names in PipeArgs).
struct RolePlan {
  uint32_t wg1 = 0, wg2 = 0, wgp = 0, wg3 = 0, wgb = 0;
  uint32_t s3_lead = 0, s3_pair = 0, s3_roles = 0, s3_xcd = 0, s3_stage = 0;
};

inline RolePlan plan_roles(const Knobs& k, const LaunchShape& l) {
  RolePlan r;
  const uint32_t PT = l.threads, wpb = PT / 64u;
  if (l.s1) r.wg1 = k.s1_wgs ? std::min(l.s1_tiles, k.s1_wgs) : l.s1_tiles;
  if (l.s2) {
    r.wg2 = std::max(1u, std::min((l.scan_threads + PT - 1) / PT, 2u * l.cu_count));
    if (k.s2_wgs) r.wg2 = std::min(r.wg2, k.s2_wgs);
  }
  // partition threads: the group applied, retention, acks; with a transport in every launch (they
  // also record each led partition's commit at the launch's end, which the next plan carries)
  if (l.s3 || l.s4 || l.acks || l.repl) r.wgp = (l.P + PT - 1) / PT;
  if (!l.s3) return r;
  const uint32_t want = std::max(1u, (l.s3_tasks + wpb - 1) / wpb);
  // default: one wave per task (the workgroups past the resident slots start as stage-1/2
  // workgroups retire); RMQ_WG3_ALL=0 fills only the slots next to the other roles (resident
  // workgroups per CU from the kernel's launch bounds) and the task waves loop over the rest
  const bool split = k.split && !l.transport;  // (the apply launch holds no stage-1/2 workgroups)
  const uint32_t slots = l.wgs_per_cu * l.cu_count, busy = (split ? 0u : r.wg1 + r.wg2) + r.wgp;
  const uint32_t room = slots > busy + l.cu_count ? slots - busy : l.cu_count;
  r.wg3 = k.wg3_all ? want : std::min(want, room);
  if (k.s3_pair && !l.transport) {  // two tasks per wave: every task has its place (no loop)
    r.s3_pair = 1;
    r.wg3 = std::max(1u, (l.s3_tasks + 2 * wpb - 1) / (2 * wpb));
  }
  if (k.s3_roles && !l.transport && !k.split) {  // loader / storer waves: a run of tasks per workgroup
    r.s3_roles = 1;
    r.s3_pair = 0;
    r.wg3 = std::max(1u, std::min(l.s3_tasks, k.s3_roles * l.cu_count));
  }
  r.wgb = k.big_wgs ? k.big_wgs : 32u * l.cu_count / wpb;  // 32 large-record waves per CU
  // dispatch order: s3_lead stage-3 workgroups, then ranking, scans and partition threads, then
  // the rest of stage 3. Round 6 default: all of stage 3 last, so the ranking and scan chains
  // start with the launch instead of in its tail, when the first stage-3 workgroups retire
  // (42.5-43.3 vs 43.7-44.0 us per launch, 20-step 34.4-34.7 vs 35.6-35.8, profiles/r06_dispatch_order.txt;
  // round 2's +2.8 % for stage 3 first no longer holds); RMQ_S3_FIRST=1 all first, RMQ_S3_LEAD=<n> n first
  r.s3_lead = k.s3_lead ? std::min(r.wg3, k.s3_lead) : k.s3_first ? r.wg3 : 0u;
  // (with every stage-3 workgroup first or every one last: one contiguous range of blocks)
  r.s3_xcd = k.s3_xcd && (r.s3_lead == r.wg3 || r.s3_lead == 0u) && !r.s3_pair ? 1u : 0u;
  r.s3_stage = k.s3_stage;
  return r;
}

// The role of a block of the launch, in dispatch order [s3_lead stage 3 | stage 1 | stage 2 |
// partition threads | rest of stage 3]: 1, 2, 3, 4 for the partition threads, 0 past the four roles
// (the large-record and catch-up workgroups behind them).
inline int role_of_block(const RolePlan& r, uint32_t block) {
  uint32_t b = block;
  if (b < r.s3_lead) return 3;
  if ((b -= r.s3_lead) < r.wg1) return 1;
  if ((b -= r.wg1) < r.wg2) return 2;
  if ((b -= r.wg2) < r.wgp) return 4;
  if ((b -= r.wgp) < r.wg3 - r.s3_lead) return 3;
  return 0;
}

}  // namespace rmq
