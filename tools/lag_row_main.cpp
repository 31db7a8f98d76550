// lag_row_main.cpp — the row arithmetic of rmq_lag (ripplemq_amd/csrc/lag_row.hpp, shared with the
// lag kernel) as a stand-alone program, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/lag_row_main.cpp -o lag_row
//   ./lag_row
// Checked against a brute-force restatement of FORMAT.md §7 "Lag" in 128-bit integers, over every
// combination of edge words: off up to 2^64 - 2, a high watermark below, at and above the log start,
// positions past 2^32 and 2^58, rings and intervals of every legal ratio, and a retained range larger
// than the ring (headroom saturates at 0). The headroom is also checked against its meaning: the
// retention rule of FORMAT.md §4 evaluated at log_end_pos + headroom keeps the record, and at 16
// bytes more evicts it.
#include <cassert>
#include <cstdio>
#include <vector>

#include "../ripplemq_amd/csrc/lag_row.hpp"

using namespace rmq;
typedef unsigned __int128 u128;
typedef std::vector<uint64_t> U64;

struct Want {
  uint64_t start_offset, records, bytes, evicted, start_pos, end_pos, headroom;
  int status;
};

// FORMAT.md §7 "Lag", steps 4 to 6, word by word.
static Want reference(uint64_t off, uint64_t hw, uint64_t lso, uint64_t sp, uint64_t ep, uint64_t lsp, uint64_t lep,
                      uint64_t S, uint32_t ilog) {
  Want w{off, 0, 0, 0, 0, 0, ~0ull, 0};
  if (off >= hw) return w;
  if (off < lso) {
    w.status = -6;
    w.start_offset = lso;
    w.evicted = lso - off;
  }
  if (hw <= w.start_offset) return w;
  w.records = hw - w.start_offset;
  w.start_pos = sp;
  w.end_pos = ep;
  w.bytes = ep - sp;
  const u128 I = (u128)1 << ilog;
  const u128 fl = ((u128)sp / I) * I;
  const u128 keep = fl > lsp ? fl : (u128)lsp;
  const bool sane = lep >= lsp && (u128)lep - lsp <= S;
  w.headroom = sane ? (uint64_t)(keep + S - lep) : 0;
  if (sane) assert(keep + S >= lep && keep + S - lep <= S);
  return w;
}

// FORMAT.md §4 at log end e: is the record at sp (a record start, so E[m].pos <= sp iff m I <= sp) evicted?
static bool evicts(uint64_t e, uint64_t sp, uint64_t lsp, uint64_t S, uint32_t ilog) {
  if (e - lsp <= S) return false;
  const uint64_t x = e - S, I = 1ull << ilog;
  const uint64_t mI = ((x + I - 1) >> ilog) << ilog;
  return mI > sp;
}

int main() {
  const uint64_t offs[] = {0, 1, 2, 99, 100, 101, 149, 150, 151, 200, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 5,
                           1ull << 58, ~0ull - 2, ~0ull - 1};
  const uint64_t bases[] = {0, 16, 4096, (1ull << 32) - 256, 1ull << 32, (1ull << 40) + 4096, 1ull << 58, (1ull << 58) + 272};
  uint64_t rows = 0, edges = 0;
  for (uint32_t ilog : {6u, 8u, 10u, 20u})
    for (uint32_t slog : {ilog + 2u, ilog + 4u, 26u})
      for (uint64_t base : bases)
        for (uint64_t retained : U64{0, 16, (1ull << slog) - 16, 1ull << slog, (1ull << slog) + 16})
          for (uint64_t lso : U64{0, 100, (1ull << 32) + 3})
            for (uint64_t hw : U64{0, 99, 100, 150, (1ull << 32) + 7, ~0ull - 1})
              for (uint64_t off : offs) {
                const uint64_t S = 1ull << slog, lsp = base, lep = base + retained;
                // positions of the two ends anywhere in the retained range, 16-byte aligned
                for (uint64_t sp : U64{lsp, lsp + ((retained / 3) & ~15ull), lep})
                  for (uint64_t ep : U64{sp, sp + (((lep - sp) / 2) & ~15ull), lep}) {
                    const LagPlan p = lag_plan(off, hw, lso);
                    const LagRow r = lag_row(p, sp, ep, lsp, lep, S, ilog);
                    const Want w = reference(off, hw, lso, sp, ep, lsp, lep, S, ilog);
                    assert(r.start_offset == w.start_offset && r.records == w.records && r.bytes == w.bytes);
                    assert(r.evicted == w.evicted && r.start_pos == w.start_pos && r.end_pos == w.end_pos);
                    assert(r.headroom == w.headroom && r.status == w.status);
                    ++rows;
                    if (!r.records || retained > S) continue;
                    // the headroom's meaning, from the present state (one evaluation)
                    assert(!evicts(lep + r.headroom, sp, lsp, S, ilog));
                    assert(evicts(lep + r.headroom + 16, sp, lsp, S, ilog));
                    ++edges;
                  }
              }
  assert(lag_headroom(1ull << 58, 1ull << 58, (1ull << 58) + 4096, 4096, 8) == 0);
  assert(lag_headroom(300, 0, 4096, 4096, 8) == 256);   // the boundary at or below the record
  assert(lag_headroom(300, 272, 4096, 4096, 8) == 272);  // the log start above that boundary
  assert(lag_headroom(0, 0, 4112, 4096, 8) == 0 && lag_headroom(0, 16, 0, 4096, 8) == 0);  // no log's state
  std::printf("lag_row: ok (%llu rows, %llu headroom edges)\n", (unsigned long long)rows, (unsigned long long)edges);
  return rows && edges ? 0 : 1;
}
