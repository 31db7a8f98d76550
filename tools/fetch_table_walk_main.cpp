// fetch_table_walk_main.cpp — the record-table walk of rmq_fetch_table
// (ripplemq_amd/csrc/fetch_table_walk.hpp: the step the table kernel shares, the scalar walk and the
// wave's windowed walk restated lane by lane) as a stand-alone program, for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/fetch_table_walk_main.cpp -o fetch_table_walk && ./fetch_table_walk
// Seeded random runs of FORMAT.md §1 records in exactly sized heap buffers, walked intact and with
// damaged length words (0, 2^32 - 1, 0xFFFFFFF0, a value that overshoots the run by one piece, a
// smaller size), with the true count and with counts that are too small and too large; the table
// goes into an exactly sized heap array of count + 1 words. Any load outside the run or store
// outside the row's words is a sanitizer report. Checked: both walks write the same words; those
// are FORMAT.md §7's reference rule computed here in bytes; every word is a multiple of 16 in
// [0, bytes], word 0 is 0 and word `count` is the run's bytes; an intact run gives the true starts.
#include <cassert>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../ripplemq_amd/csrc/fetch_table_walk.hpp"

using namespace rmq;

// FORMAT.md §7 "Record table", the reference rule, in bytes and 64-bit.
static std::vector<uint64_t> reference(const uint8_t* run, uint64_t bytes, uint64_t count) {
  std::vector<uint64_t> w(count + 1);
  uint64_t q = 0;
  for (uint64_t k = 0; k < count; ++k) {
    w[k] = q;
    if (q < bytes) {
      uint32_t len;
      std::memcpy(&len, run + q + 8, 4);
      const uint64_t nx = q + 16ull + (((uint64_t)len + 15ull) & ~15ull);
      q = nx < bytes ? nx : bytes;
    }
  }
  w[count] = bytes;
  return w;
}

static uint64_t check(const uint8_t* run, uint64_t bytes, uint64_t count) {
  const std::vector<uint64_t> want = reference(run, bytes, count);
  uint64_t* a = new uint64_t[count + 1];  // exactly the row's words
  uint64_t* b = new uint64_t[count + 1];
  uint64_t* c = new uint64_t[count + 1];
  std::memset(a, 0xA5, (count + 1) * 8);
  std::memset(b, 0x5A, (count + 1) * 8);
  std::memset(c, 0x3C, (count + 1) * 8);
  table_walk_scalar(run, bytes >> 4, count, a);
  table_walk_windows<uint64_t>(run, bytes >> 4, count, b);
  table_walk_windows<uint32_t>(run, (uint32_t)(bytes >> 4), (uint32_t)count, c);  // the kernel's index width
  for (uint64_t k = 0; k <= count; ++k) {
    assert(a[k] == want[k] && b[k] == want[k] && c[k] == want[k]);
    assert(!(a[k] & 15ull) && a[k] <= bytes);
  }
  assert((count == 0 || a[0] == 0) && a[count] == bytes);
  delete[] a;
  delete[] b;
  delete[] c;
  return count + 1;
}

int main() {
  // the step alone: exact fit, clamp, no wrap
  typedef uint64_t W;
  typedef uint32_t N;
  assert(table_next<W>(0, 0, 10) == 1 && table_next<W>(0, 1, 10) == 2 && table_next<W>(0, 16, 10) == 2 && table_next<W>(0, 17, 10) == 3);
  assert(table_next<W>(8, 16, 10) == 10 && table_next<W>(8, 17, 10) == 10 && table_next<W>(9, 0, 10) == 10);
  assert(table_next<W>(9, 0xFFFFFFFFu, 10) == 10 && table_next<W>((1ull << 28) - 2, 0xFFFFFFFFu, 1ull << 28) == 1ull << 28);
  assert(table_next<W>(5, 0xFFFFFFFFu, ~0ull) == 5ull + 1ull + (1ull << 28));
  // 32-bit indices at the largest run a fetch row can name: the same steps, no wrap
  for (N q : {0u, 1u, (1u << 28) - 2u, (1u << 28) - 1u})
    for (uint32_t len : {0u, 1u, 16u, 17u, 0xFFFFFFF0u, 0xFFFFFFFFu})
      for (N nb : {(N)(q + 1u), 1u << 28})
        assert(table_next<N>(q, len, nb) == table_next<W>(q, len, nb));
  std::mt19937_64 rng(13);
  uint64_t words = 0, runs = 0;
  for (int round = 0; round < 3000; ++round) {
    // a run of nrec records; now and then one of more than 64 pieces, an empty payload, or no record
    const uint32_t nrec = round % 50 == 0 ? 0 : 1 + rng() % (round % 7 == 0 ? 300 : 70);
    std::vector<uint32_t> lens(nrec);
    std::vector<uint64_t> starts(nrec + 1, 0);
    for (uint32_t k = 0; k < nrec; ++k) {
      const uint64_t c = rng() % 16;
      lens[k] = c == 0 ? 0 : c == 1 ? 1025 + rng() % 16000 : 1 + rng() % 300;
      starts[k + 1] = starts[k] + 16ull + (((uint64_t)lens[k] + 15ull) & ~15ull);
    }
    const uint64_t bytes = starts[nrec];
    uint8_t* run = new uint8_t[bytes ? bytes : 1];  // exactly the run (one byte for an empty one, never read)
    for (uint64_t b = 0; b < bytes; ++b) run[b] = (uint8_t)rng();
    for (uint32_t k = 0; k < nrec; ++k) {
      const uint64_t off = 1000 + k;
      std::memcpy(run + starts[k], &off, 8);
      std::memcpy(run + starts[k] + 8, &lens[k], 4);
    }
    // intact: the true starts
    {
      const std::vector<uint64_t> want = reference(run, bytes, nrec);
      for (uint32_t k = 0; k <= nrec; ++k) assert(want[k] == starts[k]);
      words += check(run, bytes, nrec);
    }
    // damaged length words, one to three per run
    for (int variant = 0; nrec && variant < 6; ++variant) {
      std::vector<uint8_t> saved(run, run + bytes);
      const uint32_t hits = 1 + rng() % 3;
      for (uint32_t h = 0; h < hits; ++h) {
        const uint32_t k = rng() % nrec;
        const uint64_t left = bytes - starts[k];  // bytes from this record's start to the run's end
        uint32_t len = 0;
        switch ((variant + h) % 6) {
          case 0: len = 0; break;
          case 1: len = 0xFFFFFFFFu; break;
          case 2: len = 0xFFFFFFF0u; break;
          case 3: len = (uint32_t)left; break;          // overshoots the run by one piece
          case 4: len = (uint32_t)(left - 16); break;   // ends exactly with the run
          default: len = lens[k] / 2; break;            // a smaller size: the walk lands inside payloads
        }
        std::memcpy(run + starts[k] + 8, &len, 4);
      }
      words += check(run, bytes, nrec);
      words += check(run, bytes, nrec / 2);
      words += check(run, bytes, nrec + 1 + rng() % 200);
      std::memcpy(run, saved.data(), bytes);
    }
    // a row whose words say records where the run has none, and a count that is wrong on an intact run
    words += check(run, 0, rng() % 5);
    words += check(run, bytes, nrec + 70);
    delete[] run;
    ++runs;
  }
  std::printf("fetch_table_walk: ok (%llu runs, %llu table words)\n", (unsigned long long)runs, (unsigned long long)words);
  return runs ? 0 : 1;
}
