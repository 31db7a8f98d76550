// repl_plan_main.cpp — the replication lists, buffer bounds and round layout
// (ripplemq_amd/csrc/repl_plan.hpp) as a stand-alone program, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/repl_plan_main.cpp -o repl_plan && ./repl_plan
// Literal cases worked by hand from the arithmetic repl_set_lists and post_round had before it
// became functions, then invariants over a seeded random sweep: one placement given to every rank of
// a world (what the handshake checks across ranks), and random landed sizes.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../ripplemq_amd/csrc/repl_plan.hpp"

using namespace rmq;

// kernels.hpp and the C header, as committed
constexpr uint32_t kMaxRemote = 4, kMaxRf = 8;                 // kMaxRemote, RMQ_MAX_RF
constexpr RegionConsts kRegion = {64, 48, 16ull << 10};        // kRegionHdr, kDirEntry, kCopyChunk
constexpr uint64_t kChunk = 16ull << 10, kVerifyRecs = 32;     // kCopyChunk, verify_records_per_task()
constexpr uint32_t N = ~0u;                                    // "not in the out list"

using V32 = std::vector<uint32_t>;
using V64 = std::vector<uint64_t>;

static int g_cases = 0, g_bad = 0;

static void fail(int line, const char* what) {
  std::fprintf(stderr, "line %d: %s\n", line, what);
  ++g_bad;
}
#define CHECK(c) ((c) ? (void)0 : fail(__LINE__, #c))

static ReplLists lists_of(uint32_t W, uint32_t me, uint32_t RF, const V32& ranks, const V32& slots, const V64& keys) {
  Placement pl;
  pl.P = (uint32_t)keys.size(), pl.RF = RF, pl.W = W, pl.me = me;
  pl.ranks = ranks.data(), pl.leader_slot = slots.data(), pl.key = keys.data();
  return plan_lists(pl, kMaxRemote, kMaxRf);
}

struct WantLists {
  V32 xo_p, xo_slot, xo_start, xi_p, xi_slot, xi_start;
  V64 keysum, keysum_in;
  V32 outidx;
  uint32_t max_remote;
  bool bad;
};
static void expect_lists(int line, const ReplLists& l, const WantLists& w) {
  const bool same = l.xo_p == w.xo_p && l.xo_slot == w.xo_slot && l.xo_start == w.xo_start && l.xi_p == w.xi_p &&
                    l.xi_slot == w.xi_slot && l.xi_start == w.xi_start && l.keysum == w.keysum &&
                    l.keysum_in == w.keysum_in && l.outidx == w.outidx && l.max_remote == w.max_remote && l.bad == w.bad;
  if (!same) fail(line, "lists differ");
  ++g_cases;
}

static void literal_lists() {
  // The base placement: W = 2, RF = 3, P = 4, leader slot 0 everywhere. Rank 0 leads 0 (both followers
  // on rank 1), follows 1 (slot 1) and 2 (slots 1, 2), holds nothing of 3. entry_hash = key * 8 + slot.
  const V32 rows = {0, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1}, slot0 = {0, 0, 0, 0};
  const V64 up = {10, 13, 16, 19}, down = {19, 16, 13, 10};
  // rank 0: out to rank 1 is partition 0's slots 1, 2 (81 + 82); in from rank 1 is (13,1) (16,1) (16,2)
  expect_lists(__LINE__, lists_of(2, 0, 3, rows, slot0, up),
               {{0, 0}, {1, 2}, {0, 0, 2}, {1, 2, 2}, {1, 1, 2}, {0, 0, 3}, {0, 163}, {0, 364},
                {N, 0, 1, N, N, N, N, N, N, N, N, N}, 2, false});
  // rank 1: the mirror image (its out list is rank 0's in list, sums included)
  expect_lists(__LINE__, lists_of(2, 1, 3, rows, slot0, up),
               {{1, 2, 2}, {1, 1, 2}, {0, 3, 3}, {0, 0}, {1, 2}, {0, 2, 2}, {364, 0}, {163, 0},
                {N, N, N, N, 0, N, N, 1, 2, N, N, N}, 2, false});
  // keys descending: the lists go by (key, slot), not by partition: partition 2 (key 13) before 1 (16)
  expect_lists(__LINE__, lists_of(2, 0, 3, rows, slot0, down),
               {{0, 0}, {1, 2}, {0, 0, 2}, {2, 2, 1}, {1, 2, 1}, {0, 0, 3}, {0, 307}, {0, 340},
                {N, 0, 1, N, N, N, N, N, N, N, N, N}, 2, false});
  expect_lists(__LINE__, lists_of(2, 1, 3, rows, slot0, down),
               {{2, 2, 1}, {1, 2, 1}, {0, 3, 3}, {0, 0}, {1, 2}, {0, 2, 2}, {340, 0}, {307, 0},
                {N, N, N, N, 2, N, N, 0, 1, N, N, N}, 2, false});
  // partition 1 led by its slot 1 (rank 0): its slots 0 and 2 join rank 0's out list (104 + 106)
  expect_lists(__LINE__, lists_of(2, 0, 3, rows, {0, 1, 0, 0}, up),
               {{0, 0, 1, 1}, {1, 2, 0, 2}, {0, 0, 4}, {2, 2}, {1, 2}, {0, 0, 2}, {0, 373}, {0, 259},
                {N, 0, 1, 2, N, 3, N, N, N, N, N, N}, 2, false});
  // a rank that leads nothing and follows nothing (rank 2 of a world of 3): empty lists, no verdict
  expect_lists(__LINE__, lists_of(3, 2, 3, rows, slot0, up),
               {{}, {}, {0, 0, 0, 0}, {}, {}, {0, 0, 0, 0}, {0, 0, 0}, {0, 0, 0}, V32(12, N), 0, false});
  // a row naming rank W: the verdict, the rest of the lists as they were
  V32 beyond = rows;
  beyond[11] = 2;
  expect_lists(__LINE__, lists_of(2, 0, 3, beyond, slot0, up),
               {{0, 0}, {1, 2}, {0, 0, 2}, {1, 2, 2}, {1, 1, 2}, {0, 0, 3}, {0, 163}, {0, 364},
                {N, 0, 1, N, N, N, N, N, N, N, N, N}, 2, true});
  // ... also where that rank is the leader: nobody lists the partition
  expect_lists(__LINE__, lists_of(2, 1, 3, {2, 1, 1}, {0}, {5}), {{}, {}, {0, 0, 0}, {}, {}, {0, 0, 0}, {0, 0}, {0, 0}, {N, N, N}, 0, true});
  // RF = 5 with four remote slots is kMaxRemote exactly (4 * 56 + 1 + 2 + 3 + 4); a fifth is refused
  expect_lists(__LINE__, lists_of(2, 0, 5, {0, 1, 1, 1, 1}, {0}, {7}),
               {{0, 0, 0, 0}, {1, 2, 3, 4}, {0, 0, 4}, {}, {}, {0, 0, 0}, {0, 234}, {0, 0}, {N, 0, 1, 2, 3}, 4, false});
  expect_lists(__LINE__, lists_of(2, 0, 6, {0, 1, 1, 1, 1, 1}, {0}, {7}),
               {{0, 0, 0, 0, 0}, {1, 2, 3, 4, 5}, {0, 0, 5}, {}, {}, {0, 0, 0}, {0, 295}, {0, 0}, {N, 0, 1, 2, 3, 4}, 5, true});
  // the per-entry spans of the acks and notices: two words per entry from the peer's first entry
  const V32 start = {0, 0, 3, 7};
  CHECK(entry_span(start, 0).word == 0 && entry_span(start, 0).bytes == 0);
  CHECK(entry_span(start, 1).word == 0 && entry_span(start, 1).bytes == 48);
  CHECK(entry_span(start, 2).word == 6 && entry_span(start, 2).bytes == 64);
  CHECK(pad16(0) == 0 && pad16(1) == 16 && pad16(16) == 16 && pad16(17) == 32);
  g_cases += 2;
}

static ReplBounds bounds_of(uint64_t G, uint64_t NR, uint64_t MB, uint64_t C, uint32_t W, uint32_t RF, uint32_t max_remote,
                            uint64_t n_out, uint64_t n_in) {
  BoundsShape s;
  s.group_max = G, s.max_batch_records = NR, s.max_batch_bytes = MB, s.max_consumers = C;
  s.W = W, s.RF = RF, s.max_remote = max_remote, s.n_out = n_out, s.n_in = n_in;
  return plan_bounds(s, kRegion);
}
static void expect_bounds(int line, const ReplBounds& b, const ReplBounds& w) {
  const bool same = b.n_out == w.n_out && b.n_in == w.n_in && b.reserve == w.reserve && b.dcap == w.dcap &&
                    b.out_cap == w.out_cap && b.in_cap == w.in_cap && b.items_cap == w.items_cap;
  if (!same) {
    std::fprintf(stderr, "line %d: got {%llu, %llu, %llu, %llu, %llu, %llu, %llu}\n", line, (unsigned long long)b.n_out,
                 (unsigned long long)b.n_in, (unsigned long long)b.reserve, (unsigned long long)b.dcap,
                 (unsigned long long)b.out_cap, (unsigned long long)b.in_cap, (unsigned long long)b.items_cap);
    ++g_bad;
  }
  ++g_cases;
}

static void literal_bounds() {
  // rec = G * (39 * NR + MB), per entry 48 + 16 + 8 C; fields: n_out, n_in, reserve, dcap, out_cap, in_cap, items_cap
  // group_max 1, no consumers, W = 2, the base placement's rank 0 (2 out, 3 in, 2 remote slots): rec 3,520;
  // dcap = 3 * 3,520 + 64 + 16 + 64 * 2 = 10,768 up to 256; in_cap = 3 * 3,520 + 64 + 32 + 64 * 3
  expect_bounds(__LINE__, bounds_of(1, 64, 1024, 0, 2, 3, 2, 2, 3), {2, 3, 3520, 11008, 22016, 10848, 5});
  // group_max 8, 4 consumers (96 per entry), W = 16, both lists empty: the max(1, n) clamps;
  // rec 28,160; dcap = 84,480 + 80 + 96 up to 256; in_cap = 15 * (84,480 + 96) + 96; items 77 + 16 + 1
  expect_bounds(__LINE__, bounds_of(8, 64, 1024, 4, 16, 3, 2, 0, 0), {1, 1, 28160, 84736, 1355776, 1268736, 94});
  // no remote slot at all (max_remote 0) still holds a reserve, a header and one entry: 3,520 + 80 + 64 = 3,664
  expect_bounds(__LINE__, bounds_of(1, 64, 1024, 0, 2, 1, 0, 0, 0), {1, 1, 3520, 3840, 7680, 3680, 3});
  // W = 1: no peer, the inbox holds the entries' rows alone
  expect_bounds(__LINE__, bounds_of(1, 64, 1024, 0, 1, 3, 0, 0, 0), {1, 1, 3520, 3840, 3840, 64, 2});
}

struct WantRound {
  V64 sn, rn, soff, region;
  V32 task0;
  uint64_t ro, smax;
  uint32_t tasks, items;
};
static void expect_round(int line, const RoundLayout& l, uint32_t W, const WantRound& w) {
  bool same = l.ro == w.ro && l.smax == w.smax && l.tasks == w.tasks && l.items == w.items && l.task0[W] == w.task0[W];
  for (uint32_t q = 0; q < W; ++q)
    same = same && l.sn[q] == w.sn[q] && l.rn[q] == w.rn[q] && l.soff[q] == w.soff[q] && l.region[q] == w.region[q] &&
           l.task0[q] == w.task0[q];
  for (uint32_t q = W; q < kPlanMaxWorld; ++q)  // nothing past the world
    same = same && !l.sn[q] && !l.rn[q] && !l.soff[q] && !l.region[q] && !l.task0[q + 1];
  if (!same) fail(line, "round layout differs");
  ++g_cases;
}

static void literal_rounds() {
  // hs: [q] {send bytes, send records}, then [W + q] {recv bytes, recv records}
  // all sizes zero: no task, no byte, the items bound is one per rank plus one per in entry
  V64 hs(8, 0);
  expect_round(__LINE__, plan_round(hs.data(), 2, 0, 11008, kVerifyRecs, 5, 3, kChunk), 2,
               {{0, 0}, {0, 0}, {0, 11008}, {0, 0}, {0, 0, 0}, 0, 0, 0, 5});
  // W = 3 seen from rank 1: its own words are ignored both ways; 50 bytes from rank 0 take 64 in the
  // inbox, 33 records two tasks; rank 2's 16 bytes follow at 64 with one task
  hs = {100, 3, 77, 9, 0, 0, 50, 33, 999, 999, 16, 1};
  expect_round(__LINE__, plan_round(hs.data(), 3, 1, 1000, kVerifyRecs, 100, 4, kChunk), 3,
               {{100, 0, 0}, {50, 0, 16}, {0, 1000, 2000}, {0, 64, 64}, {0, 2, 2, 3}, 80, 100, 3, 7});
  // record counts 0, 1, the task size and one more (0, 1, 1, 2 tasks), and records announced with no
  // bytes (no task), seen from rank 5 of 6
  hs = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 16, 1, 16, 32, 16, 33, 0, 5, 0, 0};
  expect_round(__LINE__, plan_round(hs.data(), 6, 5, 256, kVerifyRecs, 100, 0, kChunk), 6,
               {V64(6, 0), {16, 16, 16, 16, 0, 0}, {0, 256, 512, 768, 1024, 1280}, {0, 16, 32, 48, 64, 64},
                {0, 0, 1, 2, 4, 4, 4}, 64, 0, 4, 6});
  // the 32-bit cast covers the sum, not the quotient (as post_round always had it): 2^32 + 1 records are one task
  hs = {0, 0, 0, 0, 0, 0, 16, (1ull << 32) + 1};
  expect_round(__LINE__, plan_round(hs.data(), 2, 0, 256, kVerifyRecs, 100, 0, kChunk), 2,
               {{0, 0}, {0, 16}, {0, 256}, {0, 0}, {0, 0, 1}, 16, 0, 1, 2});
  // received bytes around a copy chunk: the padded size counts, so one byte short of a chunk is a
  // chunk already (2 + 1 items), 16 short is none
  for (uint64_t nb : {kChunk - 16, kChunk - 1, kChunk, kChunk + 1}) {
    hs = {0, 0, 0, 0, 0, 0, nb, 1};
    const uint64_t ro = pad16(nb);
    expect_round(__LINE__, plan_round(hs.data(), 2, 0, 256, kVerifyRecs, 100, 0, kChunk), 2,
                 {{0, 0}, {0, nb}, {0, 256}, {0, 0}, {0, 0, 1}, ro, 0, 1, nb == kChunk - 16 ? 2u : 3u});
  }
  // ... and never more items than the buffer holds
  expect_round(__LINE__, plan_round(hs.data(), 2, 0, 256, kVerifyRecs, 2, 0, kChunk), 2,
               {{0, 0}, {0, kChunk + 1}, {0, 256}, {0, 0}, {0, 0, 1}, kChunk + 16, 0, 1, 2});
  // what post_round refuses: smax > dcap, ro > in_cap (dcap 256, in_cap 64 here)
  for (uint64_t d : {0, 1}) {
    hs = {0, 0, 256 + d, 1, 0, 0, 64 + d, 1};
    const RoundLayout l = plan_round(hs.data(), 2, 0, 256, kVerifyRecs, 100, 0, kChunk);
    CHECK(l.smax == 256 + d && (l.smax > 256) == (d == 1));
    CHECK(l.ro == (d ? 80u : 64u) && (l.ro > 64) == (d == 1));
    ++g_cases;
  }
}

static void check(bool ok, const char* what, uint64_t it) {
  if (ok) return;
  std::fprintf(stderr, "sweep %llu: %s\n", (unsigned long long)it, what);
  ++g_bad;
}

static void sweep(uint64_t n) {
  std::mt19937_64 rng(0x524D5139ull);
  auto pick = [&](uint32_t hi) { return (uint32_t)(rng() % ((uint64_t)hi + 1)); };  // [0, hi]
  for (uint64_t it = 0; it < n && g_bad < 20; ++it) {
    // one placement with distinct keys, given to every rank of the world
    const uint32_t W = 1 + pick(7), RF = 1 + pick(4), P = 1 + pick(23);
    V32 ranks((size_t)P * RF), slots(P);
    V64 keys(P);
    for (uint32_t p = 0; p < P; ++p) keys[p] = 3 + 5ull * p;
    std::shuffle(keys.begin(), keys.end(), rng);
    for (uint32_t& r : ranks) r = pick(W - 1);
    for (uint32_t& s : slots) s = pick(RF - 1);
    std::vector<ReplLists> L;
    for (uint32_t me = 0; me < W; ++me) L.push_back(lists_of(W, me, RF, ranks, slots, keys));
    for (uint32_t a = 0; a < W; ++a) {
      const ReplLists& l = L[a];
      check(!l.bad, "a placement inside the world with RF <= 5 is accepted", it);
      check(l.xo_start.size() == W + 1 && l.xi_start.size() == W + 1 && l.xo_start[0] == 0 && l.xi_start[0] == 0 &&
                l.xo_start[W] == l.xo_p.size() && l.xi_start[W] == l.xi_p.size() && l.xo_p.size() == l.xo_slot.size() &&
                l.xi_p.size() == l.xi_slot.size(),
            "the start arrays begin at 0 and end at the lists' lengths", it);
      bool mono = true;
      for (uint32_t q = 0; q < W; ++q) mono = mono && l.xo_start[q] <= l.xo_start[q + 1] && l.xi_start[q] <= l.xi_start[q + 1];
      check(mono, "the start arrays are monotone", it);
      check(l.xo_start[a + 1] == l.xo_start[a] && l.xi_start[a + 1] == l.xi_start[a], "nothing to or from itself", it);
      // rank a's out list to b is rank b's in list from a
      for (uint32_t b = 0; b < W && mono; ++b) {
        const ReplLists& m = L[b];
        const uint32_t o0 = l.xo_start[b], o1 = l.xo_start[b + 1], i0 = m.xi_start[a], i1 = m.xi_start[a + 1];
        bool same = o1 - o0 == i1 - i0 && l.keysum[b] == m.keysum_in[a];
        for (uint32_t k = 0; same && k < o1 - o0; ++k)
          same = l.xo_p[o0 + k] == m.xi_p[i0 + k] && l.xo_slot[o0 + k] == m.xi_slot[i0 + k];
        check(same, "a's out list to b is b's in list from a", it);
      }
      // outidx is the inverse of the out list and ~0 elsewhere; max_remote its largest row count
      std::vector<uint32_t> inv((size_t)P * RF, N);
      for (uint32_t k = 0; k < l.xo_p.size(); ++k) inv[(size_t)l.xo_p[k] * RF + l.xo_slot[k]] = k;
      check(inv == l.outidx, "outidx inverts the out list", it);
      uint32_t most = 0;
      for (uint32_t p = 0; p < P; ++p) {
        uint32_t k = 0;
        for (uint32_t s = 0; s < RF; ++s) k += ranks[(size_t)p * RF + slots[p]] == a && ranks[(size_t)p * RF + s] != a;
        most = std::max(most, k);
      }
      check(most == l.max_remote, "max_remote is the most remote slots of a led partition", it);
    }
    // one round's landed sizes
    const uint32_t me = pick(W - 1);
    const uint64_t dcap = 256ull * (1 + pick(40)), kvr = rng() % 2 ? 32 : 64, items_cap = pick(64), n_in = pick(30);
    V64 hs(4ull * W);
    for (uint64_t& v : hs) v = rng() % 3 ? pick(70000) : 0;
    const RoundLayout r = plan_round(hs.data(), W, me, dcap, kvr, items_cap, n_in, kChunk);
    bool packed = r.region[0] == 0, prefix = r.task0[0] == 0;
    uint64_t smax = 0;
    for (uint32_t q = 0; q < W; ++q) {
      const uint64_t next = q + 1 < W ? r.region[q + 1] : r.ro;
      packed = packed && r.region[q] % 16 == 0 && next >= r.region[q] + r.rn[q] && next - r.region[q] < r.rn[q] + 16;
      prefix = prefix && r.task0[q] <= r.task0[q + 1] && (r.rn[q] || r.task0[q] == r.task0[q + 1]);
      packed = packed && r.soff[q] == q * dcap && (q != me || (!r.sn[q] && !r.rn[q]));
      smax = std::max(smax, r.sn[q]);
    }
    check(packed, "regions are 16-aligned, disjoint and packed in source order", it);
    check(prefix && r.task0[W] == r.tasks, "task0 is a monotone prefix that ends at tasks", it);
    check(r.items <= items_cap && r.items <= r.ro / kChunk + W + n_in && smax == r.smax, "items within their bound", it);
  }
}

int main(int argc, char** argv) {
  literal_lists();
  literal_bounds();
  literal_rounds();
  const int literals = g_cases;
  const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 20000;
  sweep(n);
  if (g_bad) {
    std::fprintf(stderr, "repl_plan: %d checks failed\n", g_bad);
    return 1;
  }
  // the catch-up reserve of two configurations, for the test that holds it against the oracle's
  const uint64_t configs[2][3] = {{2, 400, 48ull << 10}, {8, 4096, 1ull << 20}};
  for (const uint64_t* c : {configs[0], configs[1]})
    std::printf("bounds group_max %llu max_batch_records %llu max_batch_bytes %llu reserve %llu\n", (unsigned long long)c[0],
                (unsigned long long)c[1], (unsigned long long)c[2],
                (unsigned long long)bounds_of(c[0], c[1], c[2], 0, 2, 3, 2, 2, 3).reserve);
  std::printf("repl_plan: ok (%d cases: %d literal, %llu random placements and rounds)\n", literals + (int)n, literals,
              (unsigned long long)n);
  return 0;
}
