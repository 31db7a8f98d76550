// unpack_check_main.cpp — the structure checks and the length clamp of rmq_unpack
// (ripplemq_amd/csrc/unpack_check.hpp, shared with the unpack kernels) as a stand-alone program, for
// a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/unpack_check_main.cpp -o unpack_check
//   ./unpack_check
// Checked against a restatement of FORMAT.md §7 "Record columns" in 128-bit integers, over edge
// words: buffer sizes, positions and table indices below, at and past 2^32 and up to 2^64 - 1 (no sum
// of caller words may wrap), record counts past 2^32 for the row search and the strided capacity,
// length words of every alignment up to 2^32 - 1. A small table is also walked end to end: every
// word passing means exactly that the row is well formed, and a passing word keeps the header and
// the clamped payload inside the row's bytes.
#include <cassert>
#include <cstdio>
#include <vector>

#include "../ripplemq_amd/csrc/unpack_check.hpp"

using namespace rmq;
typedef unsigned __int128 u128;
typedef std::vector<uint64_t> U64;

static bool row_ref(uint64_t t0, uint64_t t1, uint64_t words, uint64_t recs, uint64_t out_pos, uint64_t bytes, uint64_t buf_bytes) {
  if (t0 > t1 || t1 > words) return false;
  if ((u128)t1 - t0 != (recs ? (u128)recs + 1 : 0)) return false;
  if (!recs) return true;
  return out_pos % 16 == 0 && (u128)out_pos + bytes <= buf_bytes && (u128)recs * 16 <= bytes;
}

static bool word_ref(uint64_t k, uint64_t recs, uint64_t w0, uint64_t w1, uint64_t bytes) {
  if (w0 % 16 || w1 % 16) return false;
  if (k == 0 && w0 != 0) return false;
  if ((u128)w0 + 16 > w1 || w1 > bytes) return false;
  return k + 1 != recs || w1 == bytes;
}

// A whole row by the definition: words start at 0, multiples of 16, steps of at least 16, end at bytes.
static bool table_ref(const U64& w, uint64_t bytes) {
  if (w.size() < 2 || w.front() != 0 || w.back() != bytes) return false;
  for (size_t i = 0; i < w.size(); ++i)
    if (w[i] % 16 || (i && (w[i] <= w[i - 1] || w[i] - w[i - 1] < 16))) return false;
  return true;
}

int main() {
  const U64 edge = {0, 1, 15, 16, 17, 32, 48, 4096, (1ull << 32) - 16, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 16,
                    (1ull << 40) + 32, (1ull << 63), ~0ull - 31, ~0ull - 15, ~0ull - 1, ~0ull};
  uint64_t rows = 0, words = 0, lens = 0, finds = 0;
  // rows
  for (uint64_t t0 : edge)
    for (uint64_t d : U64{0, 1, 2, 3, 1ull << 32, (1ull << 32) + 1})
      for (uint64_t rw : edge)
        for (uint64_t recs : U64{0, 1, 2, (1ull << 32) - 1, 1ull << 32})
          for (uint64_t op : edge)
            for (uint64_t nb : U64{0, 16, 32, 48, (1ull << 32) - 16, 1ull << 36})
              for (uint64_t bb : edge) {
                const uint64_t t1 = t0 + d;  // (may wrap: then t0 > t1 and both say no)
                assert(unpack_row_ok(t0, t1, rw, recs, op, nb, bb) == row_ref(t0, t1, rw, recs, op, nb, bb));
                ++rows;
              }
  // words
  for (uint64_t k : U64{0, 1, 2, (1ull << 32) - 1, 1ull << 32})
    for (uint64_t recs : U64{k + 1, k + 2, (1ull << 33)})
      for (uint64_t w0 : edge)
        for (uint64_t w1 : edge)
          for (uint64_t nb : edge) {
            const bool ok = unpack_word_ok(k, recs, w0, w1, nb);
            assert(ok == word_ref(k, recs, w0, w1, nb));
            if (ok) assert(w1 - w0 >= 16 && w0 + 16 <= nb);  // the header lies inside the row's bytes
            ++words;
          }
  // every word passing is the row passing
  const uint64_t steps[] = {0, 8, 16, 24, 32, 48};
  for (uint64_t a : steps)
    for (uint64_t b : steps)
      for (uint64_t c : steps)
        for (uint64_t start : U64{0, 16})
          for (uint64_t nb : U64{0, 16, 48, 64, 96, 112}) {
            const U64 w = {start, start + a, start + a + b, start + a + b + c};
            bool all = true;
            for (uint64_t k = 0; k < 3; ++k) all = all && unpack_word_ok(k, 3, w[k], w[k + 1], nb);
            assert(all == table_ref(w, nb));
            ++words;
          }
  // the clamp: len never passes the extent, the mismatch is the definition's
  for (uint64_t ext : U64{16, 32, 48, 4112, 1ull << 32, (1ull << 32) + 16, (1ull << 36)})
    for (uint64_t hl : U64{0, 1, 15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 0xFFFFFFF0ull, 0xFFFFFFFFull}) {
      bool mis = false;
      const uint32_t len = unpack_len((uint32_t)hl, ext, &mis);
      const u128 want = (u128)hl < (u128)ext - 16 ? hl : (u128)ext - 16;
      assert(len == (uint64_t)(want < 0xFFFFFFFFull ? want : 0xFFFFFFFFull) && (uint64_t)len + 16 <= ext);
      assert(mis == ((u128)16 + (((u128)hl + 15) / 16) * 16 != ext));
      ++lens;
    }
  // the row search: record counts past 2^32, rows that own nothing between owners
  const U64 first = {0, 0, 5, 5, 5, (1ull << 32) + 7, (1ull << 32) + 7, (1ull << 33), (1ull << 33) + 1};
  const uint32_t n = (uint32_t)first.size() - 1;
  for (uint64_t j : U64{0, 1, 4, 5, 6, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 6, (1ull << 32) + 7, (1ull << 33) - 1, 1ull << 33}) {
    const uint32_t r = unpack_row_of(j, n, [&](uint32_t i) {
      assert(i >= 1 && i < n);
      return first[i];
    });
    assert(r < n && first[r] <= j && j < first[r + 1]);
    ++finds;
  }
  assert(unpack_row_of(3, 1, [&](uint32_t) { assert(false); return 0ull; }) == 0);  // one row: nothing is read
  // the strided capacity where R * stride does not fit in 64 bits
  for (uint64_t R : U64{0, 1, 1ull << 32, (1ull << 33) + 1, ~0ull})
    for (uint32_t st : {0u, 1u, 17u, 128u, 0xFFFFFFFFu})
      for (uint64_t cap : edge)
        assert(unpack_strided_fits(R, st, cap) == ((u128)R * st <= cap));
  assert(unpack_row_records(7, 0) == 7 && unpack_row_records(7, -6) == 0 && unpack_row_records(0, 0) == 0);
  std::printf("unpack_check: ok (%llu rows, %llu words, %llu lengths, %llu searches)\n", (unsigned long long)rows,
              (unsigned long long)words, (unsigned long long)lens, (unsigned long long)finds);
  return rows && words && lens && finds ? 0 : 1;
}
