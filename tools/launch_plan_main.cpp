// launch_plan_main.cpp — the role grid of a pipeline launch (ripplemq_amd/csrc/launch_plan.hpp) as a
// stand-alone program, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/launch_plan_main.cpp -o launch_plan && ./launch_plan
// Literal plans worked by hand from the arithmetic launch_stages had before the plan became a
// function (256 CUs, both workgroup sizes, every knob that moves the grid with a case it changes
// and one it must not), then invariants over a seeded random sweep of shapes and knobs.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../ripplemq_amd/csrc/launch_plan.hpp"

using namespace rmq;

constexpr uint32_t kCus = 256;
constexpr uint32_t kWavesPerSimd = 4;  // RMQ_PIPE_WAVES_PER_SIMD of pipeline.hip
constexpr uint32_t kMaxGroupTiles = 512, kAllTasks = kMaxGroupTiles * 1024 / 32;  // 16,384 tasks of 32 records

static uint32_t wgs_per_cu(uint32_t threads) { return kWavesPerSimd * 4u / (threads / 64u); }  // pipeline_wgs_per_cu

// Every stage present, no transport, 256-thread workgroups (4 resident per CU: 1,024 slots).
static LaunchShape shape(uint32_t P, uint32_t tiles, uint32_t tasks) {
  LaunchShape l;
  l.P = P, l.cu_count = kCus, l.threads = 256, l.wgs_per_cu = wgs_per_cu(256);
  l.scan_threads = P * 16;  // one column per group, 16 lanes each (RMQ_SCAN_COLS, RMQ_SCAN_LANES as committed)
  l.s1 = l.s2 = l.s3 = l.s4 = true;
  l.s1_tiles = tiles, l.s3_tasks = tasks;
  return l;
}

// The same on a rank that leads partitions with a remote replica: 512 threads, 2 resident per CU.
static LaunchShape xshape(uint32_t P, uint32_t tiles, uint32_t tasks) {
  LaunchShape l = shape(P, tiles, tasks);
  l.threads = 512, l.wgs_per_cu = wgs_per_cu(512);
  l.transport = l.repl = true;
  return l;
}

static int g_line = 0, g_bad = 0;

static void expect_at(int line, const Knobs& k, const LaunchShape& l, const RolePlan& w) {
  const RolePlan r = plan_roles(k, l);
  const bool same = r.wg1 == w.wg1 && r.wg2 == w.wg2 && r.wgp == w.wgp && r.wg3 == w.wg3 && r.wgb == w.wgb &&
                    r.s3_lead == w.s3_lead && r.s3_pair == w.s3_pair && r.s3_roles == w.s3_roles &&
                    r.s3_xcd == w.s3_xcd && r.s3_stage == w.s3_stage;
  if (!same) {
    std::fprintf(stderr, "line %d: got {%u, %u, %u, %u, %u, %u, %u, %u, %u, %u}\n", line, r.wg1, r.wg2, r.wgp, r.wg3,
                 r.wgb, r.s3_lead, r.s3_pair, r.s3_roles, r.s3_xcd, r.s3_stage);
    ++g_bad;
  }
  ++g_line;
}
// the plan's fields in order: wg1, wg2, wgp, wg3, wgb, s3_lead, s3_pair, s3_roles, s3_xcd, s3_stage
#define EXPECT(k, l, ...) expect_at(__LINE__, k, l, RolePlan{__VA_ARGS__})

static Knobs knob(uint32_t Knobs::*m, uint32_t v) {
  Knobs k;
  k.*m = v;
  return k;
}

static void literal_plans() {
  const Knobs d;
  // default knobs: P at the scan grid's edges (one 16-lane group per column: wg2 = ceil(P / 16) of
  // 256 threads, at most 2 per CU; wgp = ceil(P / 256)), tiles 0 / 1 / all, tasks 0 / 1 / 4 / 5 / all
  EXPECT(d, shape(1, 0, 0), 0, 1, 1, 1, 2048, 0, 0, 0, 1, 1);
  EXPECT(d, shape(255, 1, 1), 1, 16, 1, 1, 2048, 0, 0, 0, 1, 1);
  EXPECT(d, shape(256, 512, 4), 512, 16, 1, 1, 2048, 0, 0, 0, 1, 1);
  EXPECT(d, shape(257, 512, 5), 512, 17, 2, 2, 2048, 0, 0, 0, 1, 1);
  EXPECT(d, shape(65536, 512, kAllTasks), 512, 512, 256, 4096, 2048, 0, 0, 0, 1, 1);
  // 512-thread workgroups: wg2 = ceil(P / 32), wgp = ceil(P / 512), 8 tasks per workgroup, 1,024 big
  EXPECT(d, xshape(1, 0, 0), 0, 1, 1, 1, 1024, 0, 0, 0, 1, 1);
  EXPECT(d, xshape(255, 1, 8), 1, 8, 1, 1, 1024, 0, 0, 0, 1, 1);
  EXPECT(d, xshape(256, 1, 9), 1, 8, 1, 2, 1024, 0, 0, 0, 1, 1);
  EXPECT(d, xshape(257, 512, 1), 512, 9, 1, 1, 1024, 0, 0, 0, 1, 1);
  EXPECT(d, xshape(65536, 512, kAllTasks), 512, 512, 128, 2048, 1024, 0, 0, 0, 1, 1);
  // stages absent: no role without its group; the partition threads run for stage 3, stage 4, acks
  // or any transport
  LaunchShape l = shape(257, 512, 5);
  l.s2 = l.s3 = l.s4 = false;
  EXPECT(d, l, 512, 0, 0, 0, 0, 0, 0, 0, 0, 0);
  l.s4 = true;
  EXPECT(d, l, 512, 0, 2, 0, 0, 0, 0, 0, 0, 0);
  l.s4 = false, l.acks = true;
  EXPECT(d, l, 512, 0, 2, 0, 0, 0, 0, 0, 0, 0);
  l.acks = false, l.repl = true;
  EXPECT(d, l, 512, 0, 2, 0, 0, 0, 0, 0, 0, 0);
  l = shape(257, 512, 5);
  l.s1 = false;  // (its tiles are not looked at)
  EXPECT(d, l, 0, 17, 2, 2, 2048, 0, 0, 0, 1, 1);

  // RMQ_WG3_ALL=0: stage 3 fills the slots the other roles leave (1,024 - busy), at least one per CU
  Knobs k = knob(&Knobs::wg3_all, 0);
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 2, 2048, 0, 0, 0, 1, 1);  // (2 fit: unchanged)
  EXPECT(k, shape(256, 1, kAllTasks), 1, 16, 1, 1006, 2048, 0, 0, 0, 1, 1);  // 1,024 - 18
  EXPECT(k, shape(65536, 512, kAllTasks), 512, 512, 256, 256, 2048, 0, 0, 0, 1, 1);  // busy 1,280: one per CU
  l = shape(65536, 512, kAllTasks);
  l.s2 = false;  // busy 768 = slots - CUs exactly: not more than a CU's worth left, one per CU
  EXPECT(k, l, 512, 0, 256, 256, 2048, 0, 0, 0, 1, 1);
  l.s1_tiles = 511;  // busy 767: 257 left
  EXPECT(k, l, 511, 0, 256, 257, 2048, 0, 0, 0, 1, 1);
  EXPECT(k, xshape(256, 1, kAllTasks), 1, 8, 1, 502, 1024, 0, 0, 0, 1, 1);  // 512 slots - 10

  // RMQ_S3_FIRST=1: every stage-3 workgroup first; nothing to lead without a stage 3
  k = knob(&Knobs::s3_first, 1);
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 2, 2048, 2, 0, 0, 1, 1);
  EXPECT(k, shape(65536, 512, kAllTasks), 512, 512, 256, 4096, 2048, 4096, 0, 0, 1, 1);
  l = shape(257, 512, 5);
  l.s3 = false;
  EXPECT(k, l, 512, 17, 2, 0, 0, 0, 0, 0, 0, 0);
  // RMQ_S3_LEAD=5: five of them first (two ranges of blocks: no XCD ranges), all of them if fewer
  k = knob(&Knobs::s3_lead, 5);
  EXPECT(k, shape(65536, 512, kAllTasks), 512, 512, 256, 4096, 2048, 5, 0, 0, 0, 1);
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 2, 2048, 2, 0, 0, 1, 1);
  EXPECT(k, shape(256, 1, 20), 1, 16, 1, 5, 2048, 5, 0, 0, 1, 1);
  EXPECT(k, l, 512, 17, 2, 0, 0, 0, 0, 0, 0, 0);
  k.s3_first = 1;  // (the count wins over "all first")
  EXPECT(k, shape(65536, 512, kAllTasks), 512, 512, 256, 4096, 2048, 5, 0, 0, 0, 1);
  k = knob(&Knobs::s3_xcd, 0);
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 2, 2048, 0, 0, 0, 0, 1);
  k = knob(&Knobs::s3_stage, 0);
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 2, 2048, 0, 0, 0, 1, 0);

  // RMQ_S3_PAIR=1: two tasks per wave (8 per workgroup), no XCD ranges
  k = knob(&Knobs::s3_pair, 1);
  EXPECT(k, shape(65536, 512, kAllTasks), 512, 512, 256, 2048, 2048, 0, 1, 0, 0, 1);
  EXPECT(k, shape(257, 512, 9), 512, 17, 2, 2, 2048, 0, 1, 0, 0, 1);
  EXPECT(k, shape(257, 512, 0), 512, 17, 2, 1, 2048, 0, 1, 0, 0, 1);
  EXPECT(k, l, 512, 17, 2, 0, 0, 0, 0, 0, 0, 0);  // no stage 3: nothing paired
  // RMQ_S3_ROLES=k: a workgroup per task, at most k per CU; it wins over the pairs
  k = knob(&Knobs::s3_roles, 1);
  EXPECT(k, shape(65536, 512, kAllTasks), 512, 512, 256, 256, 2048, 0, 0, 1, 1, 1);
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 5, 2048, 0, 0, 1, 1, 1);
  EXPECT(k, shape(257, 512, 0), 512, 17, 2, 1, 2048, 0, 0, 1, 1, 1);
  EXPECT(k, l, 512, 17, 2, 0, 0, 0, 0, 0, 0, 0);
  k.s3_pair = 1;
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 5, 2048, 0, 0, 1, 1, 1);
  k = knob(&Knobs::s3_roles, 4);
  EXPECT(k, shape(65536, 512, kAllTasks), 512, 512, 256, 1024, 2048, 0, 0, 1, 1, 1);
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 5, 2048, 0, 0, 1, 1, 1);

  // RMQ_SPLIT=1: the apply launch holds no ranking workgroups (only RMQ_WG3_ALL=0 sees it), and
  // the loader / storer waves are off
  k = knob(&Knobs::split, 1);
  EXPECT(k, shape(65536, 512, kAllTasks), 512, 512, 256, 4096, 2048, 0, 0, 0, 1, 1);  // unchanged
  k.wg3_all = 0;
  EXPECT(k, shape(256, 1, kAllTasks), 1, 16, 1, 1023, 2048, 0, 0, 0, 1, 1);  // 1,024 - 1 (1,006 unsplit)
  k = knob(&Knobs::split, 1);
  k.s3_roles = 1;
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 2, 2048, 0, 0, 0, 1, 1);  // roles ignored
  k.s3_pair = 1;
  EXPECT(k, shape(257, 512, 9), 512, 17, 2, 2, 2048, 0, 1, 0, 0, 1);  // the pairs are not

  // RMQ_S1_WGS, RMQ_S2_WGS: caps, never more than the uncapped count
  k = knob(&Knobs::s1_wgs, 1);
  EXPECT(k, shape(257, 512, 5), 1, 17, 2, 2, 2048, 0, 0, 0, 1, 1);
  EXPECT(k, shape(257, 1, 5), 1, 17, 2, 2, 2048, 0, 0, 0, 1, 1);
  EXPECT(k, shape(257, 0, 5), 0, 17, 2, 2, 2048, 0, 0, 0, 1, 1);
  k = knob(&Knobs::s1_wgs, 37);
  EXPECT(k, shape(257, 512, 5), 37, 17, 2, 2, 2048, 0, 0, 0, 1, 1);
  EXPECT(k, shape(257, 1, 5), 1, 17, 2, 2, 2048, 0, 0, 0, 1, 1);
  k = knob(&Knobs::s2_wgs, 1);
  EXPECT(k, shape(257, 512, 5), 512, 1, 2, 2, 2048, 0, 0, 0, 1, 1);
  EXPECT(k, shape(1, 0, 0), 0, 1, 1, 1, 2048, 0, 0, 0, 1, 1);
  k = knob(&Knobs::s2_wgs, 3);
  EXPECT(k, shape(257, 512, 5), 512, 3, 2, 2, 2048, 0, 0, 0, 1, 1);
  EXPECT(k, shape(1, 0, 0), 0, 1, 1, 1, 2048, 0, 0, 0, 1, 1);
  // RMQ_BIG_WGS=3: with a stage 3 only
  k = knob(&Knobs::big_wgs, 3);
  EXPECT(k, shape(257, 512, 5), 512, 17, 2, 2, 3, 0, 0, 0, 1, 1);
  EXPECT(k, xshape(257, 512, 5), 512, 9, 1, 1, 3, 0, 0, 0, 1, 1);
  EXPECT(k, l, 512, 17, 2, 0, 0, 0, 0, 0, 0, 0);

  // a transport with remote replicas: pairs, loader / storer waves and the split are all ignored
  k = Knobs();
  k.s3_pair = 1;
  EXPECT(k, xshape(257, 512, 9), 512, 9, 1, 2, 1024, 0, 0, 0, 1, 1);
  k = knob(&Knobs::s3_roles, 4);
  EXPECT(k, xshape(257, 512, 9), 512, 9, 1, 2, 1024, 0, 0, 0, 1, 1);
  k = knob(&Knobs::split, 1);
  k.wg3_all = 0;
  EXPECT(k, xshape(256, 1, kAllTasks), 1, 8, 1, 502, 1024, 0, 0, 0, 1, 1);  // busy counts the ranking roles
  k.s3_pair = k.s3_roles = 1;
  EXPECT(k, xshape(65536, 512, kAllTasks), 512, 512, 128, 256, 1024, 0, 0, 0, 1, 1);  // busy 1,152: one per CU
}

static void check(bool ok, const char* what, uint64_t it) {
  if (ok) return;
  std::fprintf(stderr, "sweep %llu: %s\n", (unsigned long long)it, what);
  ++g_bad;
}

static void sweep(uint64_t n) {
  std::mt19937_64 rng(0x524D5131ull);
  auto pick = [&](uint32_t hi) { return (uint32_t)(rng() % ((uint64_t)hi + 1)); };  // [0, hi]
  auto some = [&](uint32_t hi) { return rng() % 3 ? 0u : pick(hi); };                // mostly the default 0
  for (uint64_t it = 0; it < n && g_bad < 20; ++it) {
    Knobs k;
    k.wg3_all = pick(1), k.s1_wgs = some(600), k.s2_wgs = some(600), k.big_wgs = some(5000);
    k.s3_first = some(1), k.s3_lead = some(5000), k.split = some(2), k.s3_pair = some(1), k.s3_roles = some(8);
    k.s3_xcd = pick(1), k.s3_stage = pick(1);
    LaunchShape l;
    l.P = 1 + (rng() % 8 ? pick(1023) : pick(65535));
    l.scan_threads = l.P * 16;
    l.cu_count = rng() % 4 ? kCus : 1 + pick(511);
    l.repl = rng() % 3 == 0;
    l.transport = l.repl && rng() % 2;
    l.acks = l.transport && rng() % 2;
    l.threads = l.transport ? 512 : 256;
    l.wgs_per_cu = wgs_per_cu(l.threads);
    l.s1 = rng() % 4, l.s2 = rng() % 4, l.s3 = rng() % 4, l.s4 = rng() % 4;
    l.s1_tiles = l.s1 ? (rng() % 2 ? pick(8) : pick(kMaxGroupTiles)) : 0;
    l.s3_tasks = l.s3 ? (rng() % 2 ? pick(40) : pick(kAllTasks)) : 0;
    const RolePlan r = plan_roles(k, l);
    check(r.s3_lead <= r.wg3, "s3_lead <= wg3", it);
    check(!r.s3_xcd || ((r.s3_lead == 0 || r.s3_lead == r.wg3) && !r.s3_pair), "s3_xcd only for one range, unpaired", it);
    check(!r.s3_roles || !r.s3_pair, "s3_roles implies no pairs", it);
    check(!l.s3 || r.wg3 >= 1, "a stage 3 has a workgroup", it);
    check(l.s3 || (r.wg3 == 0 && r.wgb == 0 && r.s3_lead == 0), "no stage 3, no stage-3 workgroups", it);
    check(r.wg2 <= 2 * l.cu_count, "wg2 <= 2 per CU", it);
    check(l.s2 == (r.wg2 != 0) && l.s1_tiles >= r.wg1, "ranking roles only with their groups", it);
    check((r.wgp == 0) == !(l.s3 || l.s4 || l.acks || l.repl), "partition threads exactly when needed", it);
    uint32_t count[5] = {0, 0, 0, 0, 0};
    const uint32_t blocks = r.wg1 + r.wg2 + r.wgp + r.wg3;
    bool ordered = true;
    int stage = -1;  // position in the dispatch order: lead 3, 1, 2, 4, rest of 3, then 0
    for (uint32_t b = 0; b < blocks + 3; ++b) {
      const int role = role_of_block(r, b);
      count[role]++;
      const int pos = role == 3 ? (b < r.s3_lead ? 0 : 4) : role == 1 ? 1 : role == 2 ? 2 : role == 4 ? 3 : 5;
      ordered = ordered && pos >= stage;
      stage = pos;
    }
    check(count[1] == r.wg1 && count[2] == r.wg2 && count[4] == r.wgp && count[3] == r.wg3 && count[0] == 3,
          "role_of_block gives each role its count", it);
    check(ordered, "role_of_block follows the dispatch order", it);
  }
}

int main(int argc, char** argv) {
  literal_plans();
  const int literals = g_line;
  const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 300000;
  sweep(n);
  if (g_bad) {
    std::fprintf(stderr, "launch_plan: %d checks failed\n", g_bad);
    return 1;
  }
  std::printf("launch_plan: ok (%d literal plans, %llu random shapes)\n", literals, (unsigned long long)n);
  return 0;
}
