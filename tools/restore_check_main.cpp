// restore_check_main.cpp — rmq_restore's host-side item checks and staging plan
// (ripplemq_amd/csrc/restore_check.hpp) as a stand-alone program, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/restore_check_main.cpp -o restore_check && ./restore_check
// Every §11 host check once, then seeded random items whose accepted spans are staged the way the
// engine stages a host buffer (one copy of the covering span of the runs, one of the tables) into
// exactly sized heap buffers, and read back through the rebased addresses: any address the plan
// derives outside the caller's arrays or the scratch is a sanitizer report.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <random>

#include "../ripplemq_amd/csrc/restore_check.hpp"

using namespace rmq;

static const uint32_t P = 8;
static const uint64_t S = 4096;
static bool g_pristine[P], g_local[P];

static RestorePart part(uint32_t p) { return RestorePart{S, g_pristine[p], g_local[p]}; }

static rmq_restore_item good(uint32_t p) {
  rmq_restore_item it{};
  it.pidx = p, it.first_offset = 10, it.first_pos = 160, it.count = 4, it.bytes = 128, it.buf_pos = 32;
  it.table_start = 3, it.commit = 12;
  return it;
}

static int32_t one(const rmq_restore_item& it, uint64_t buf_bytes = 1024, uint64_t words = 64) {
  return restore_plan(1, &it, P, buf_bytes, words, part).status[0];
}

int main() {
  for (uint32_t p = 0; p < P; ++p) g_pristine[p] = g_local[p] = true;
  rmq_restore_item it = good(1);
  assert(one(it) == RMQ_OK);
#define BAD(expr, want) do { it = good(1); expr; assert(one(it) == (want)); } while (0)
  BAD(it.pidx = P, RMQ_ENOPART);
  BAD(it.pidx = ~0u, RMQ_ENOPART);
  BAD(it.flags = 1, RMQ_EINVAL);
  BAD(it.first_pos = 8, RMQ_EINVAL);
  BAD(it.buf_pos = 8, RMQ_EINVAL);
  BAD(it.bytes = 120, RMQ_EINVAL);
  BAD(it.count = 9, RMQ_EINVAL);
  BAD((it.count = 0, it.commit = 10), RMQ_EINVAL);
  BAD(it.buf_pos = 1024 - 112, RMQ_EINVAL);
  BAD(it.buf_pos = ~0ull & ~15ull, RMQ_EINVAL);
  BAD(it.bytes = ~0ull & ~15ull, RMQ_EINVAL);
  BAD(it.table_start = 60, RMQ_EINVAL);
  BAD(it.table_start = ~0ull, RMQ_EINVAL);
  BAD(it.count = ~0ull, RMQ_EINVAL);
  BAD(it.commit = 9, RMQ_EINVAL);
  BAD(it.commit = 15, RMQ_EINVAL);
  BAD((it.first_offset = kRestoreMax - 2, it.commit = it.first_offset), RMQ_EINVAL);
  BAD((it.first_offset = ~0ull, it.commit = it.first_offset), RMQ_EINVAL);
  BAD(it.first_pos = kRestoreMax - 16, RMQ_EINVAL);
  BAD(it.first_pos = ~0ull & ~15ull, RMQ_EINVAL);
  it = good(1), it.bytes = S + 16, it.count = 4;
  assert(one(it, 2 * S) == RMQ_ENOSPC);
  it = good(1), it.bytes = S;
  assert(one(it, 2 * S) == RMQ_OK);  // the ring itself, not the ring less an interval
  g_pristine[1] = false;
  assert(one(good(1)) == RMQ_EINVAL);
  g_pristine[1] = true, g_local[1] = false;
  assert(one(good(1)) == RMQ_EINVAL);
  g_local[1] = true;
  {  // an empty run, a duplicate, refused rows between accepted ones
    rmq_restore_item v[5] = {good(1), good(P), good(1), good(2), good(3)};
    v[3].count = 0, v[3].bytes = 0, v[3].commit = 10, v[3].buf_pos = 1024, v[3].table_start = 63;
    v[4].buf_pos = 512, v[4].table_start = 20;
    const RestorePlan pl = restore_plan(5, v, P, 1024, 64, part);
    assert(pl.status[0] == RMQ_OK && pl.status[1] == RMQ_ENOPART && pl.status[2] == RMQ_EINVAL && pl.status[3] == RMQ_OK &&
           pl.status[4] == RMQ_OK);
    assert(pl.accepted.size() == 3 && pl.rbase.size() == 4 && pl.rbase[3] == 8 && pl.bytes == 256);
    assert(pl.buf_lo == 32 && pl.buf_hi == 640 && pl.tab_lo == 3 && pl.tab_hi == 64);
    assert(restore_return(pl.status) == RMQ_ENOPART);
  }
  // seeded items over caller arrays of exact size, staged as the engine stages them
  std::mt19937_64 rng(11);
  uint64_t accepted = 0;
  for (int round = 0; round < 2000; ++round) {
    const uint64_t buf_bytes = 16 * (rng() % 600), words = rng() % 200;
    std::vector<uint8_t> buf(buf_bytes);
    std::vector<uint64_t> tab(words);
    for (auto& b : buf) b = (uint8_t)rng();
    for (auto& w : tab) w = rng();
    const uint32_t n = 1 + rng() % 6;
    std::vector<rmq_restore_item> v(n);
    for (auto& x : v) {
      x = rmq_restore_item{};
      x.pidx = rng() % (P + 1);
      x.count = rng() % 5 ? rng() % 40 : rng();
      x.bytes = rng() % 7 ? 16 * (rng() % 300) : rng();
      x.buf_pos = rng() % 7 ? 16 * (rng() % 600) : rng();
      x.table_start = rng() % 7 ? rng() % 200 : rng();
      x.first_offset = rng() % 9 ? rng() % 1000 : rng();
      x.first_pos = rng() % 9 ? 16 * (rng() % 1000) : rng();
      x.commit = x.first_offset + (rng() % 3 ? x.count : rng() % 50);
      x.flags = rng() % 20 ? 0 : 1;
    }
    const RestorePlan pl = restore_plan(n, v.data(), P, buf_bytes, words, part);
    std::vector<uint8_t> dbuf(pl.buf_hi - pl.buf_lo);
    std::vector<uint64_t> dtab(pl.tab_hi - pl.tab_lo);
    if (!dbuf.empty()) std::memcpy(dbuf.data(), buf.data() + pl.buf_lo, dbuf.size());
    if (!dtab.empty()) std::memcpy(dtab.data(), tab.data() + pl.tab_lo, dtab.size() * 8);
    uint64_t sum = 0;
    for (size_t k = 0; k < pl.accepted.size(); ++k) {
      const rmq_restore_item& x = v[pl.accepted[k]];
      const uint8_t* run = dbuf.data() + (x.bytes ? x.buf_pos - pl.buf_lo : 0);
      const uint64_t* t = dtab.data() + (x.table_start - pl.tab_lo);
      for (uint64_t b = 0; b < x.bytes; ++b) sum += run[b];
      for (uint64_t w = 0; w <= x.count; ++w) sum += t[w];
      assert(pl.rbase[k + 1] - pl.rbase[k] == x.count);
      ++accepted;
    }
    (void)sum;
  }
  std::printf("restore_check: ok (%llu random items accepted and staged)\n", (unsigned long long)accepted);
  return accepted ? 0 : 1;
}
