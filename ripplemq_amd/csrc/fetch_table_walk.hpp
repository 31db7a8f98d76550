// fetch_table_walk.hpp — the step of the record-table walk (FORMAT.md §7 "Record table"), shared by
// the table kernel of fetch.hip and a stand-alone host program that runs the same walk over damaged
// runs under the sanitizers (tools/fetch_table_walk_main.cpp). Plain C++: no device, no engine.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RMQ_TABLE_HD __host__ __device__
#else
#define RMQ_TABLE_HD
#endif

namespace rmq {

// Positions in 16-byte pieces. A record starts at piece q < nb16 of a run of nb16 pieces and its
// length word is len: the piece the next record starts at, never past the run's end. T = uint64_t
// holds for any run: a length word near 2^32 adds 2^28 pieces and cannot wrap. T = uint32_t holds
// for nb16 <= 2^28 (a fetch row's bytes are a 32-bit word, so its runs are below that): q < 2^28
// and at most 2^28 + 1 pieces more stay below 2^30, so the 32-bit sum cannot wrap either.
template <typename T>
RMQ_TABLE_HD inline T table_next(T q, uint32_t len, T nb16) {
  const T nx = q + (T)1 + (T)(len >> 4) + (T)((len & 15u) ? 1u : 0u);
  return nx < nb16 ? nx : nb16;
}

// The length word of piece `piece` of the run at base, or 0 for a piece at or past the run's end:
// the one load of the walk, and no byte outside the run is ever read.
RMQ_TABLE_HD inline uint32_t table_len_at(const uint8_t* base, uint64_t nb16, uint64_t piece) {
  return piece < nb16 ? *reinterpret_cast<const uint32_t*>(base + 16ull * piece + 8ull) : 0u;
}

// The table of one run, record after record (the reference of the wave's walk): words[0 .. count]
// = byte positions of records 0 .. count - 1, then the run's bytes; once the walk reaches the end of
// the run early (a damaged length word) the words left are the run's bytes.
inline void table_walk_scalar(const uint8_t* base, uint64_t nb16, uint64_t count, uint64_t* words) {
  uint64_t q = 0;
  for (uint64_t k = 0; k < count; ++k) {
    words[k] = 16ull * q;
    if (q < nb16) q = table_next<uint64_t>(q, table_len_at(base, nb16, q), nb16);
  }
  words[count] = 16ull * nb16;
}

// The same table as the wave computes it, lane by lane on the host: the length words of 64 pieces
// per window (lane l holds piece 64 k + l), the next window loaded ahead, at most 64 record starts
// per round kept a lane each and stored together, the words after an early end filled 64 at a time.
// T: the kernel's 32-bit piece indices (nb16 <= 2^28, count < 2^32), or 64-bit ones.
template <typename T>
inline void table_walk_windows(const uint8_t* base, T nb16, T count, uint64_t* words) {
  uint32_t W0[64], W1[64];
  T q = 0, done = 0, wk = 0;
  for (uint32_t l = 0; l < 64; ++l) {
    W0[l] = table_len_at(base, nb16, l);
    W1[l] = table_len_at(base, nb16, 64ull + l);
  }
  while (done < count && q < nb16) {
    T myq[64] = {};
    uint32_t nrec = 0;
    const uint32_t lim = count - done < (T)64 ? (uint32_t)(count - done) : 64u;
    while (nrec < lim && q < nb16) {
      const T k = q >> 6;
      if (k != wk) {
        for (uint32_t l = 0; l < 64; ++l) {
          W0[l] = k == wk + (T)1 ? W1[l] : table_len_at(base, nb16, 64ull * k + l);
          W1[l] = table_len_at(base, nb16, 64ull * ((uint64_t)k + 1ull) + l);
        }
        wk = k;
      }
      myq[nrec] = q;
      q = table_next<T>(q, W0[q & (T)63], nb16);
      ++nrec;
    }
    for (uint32_t l = 0; l < nrec; ++l) words[(uint64_t)done + l] = 16ull * myq[l];
    done += (T)nrec;
  }
  for (uint64_t k = done; k <= (uint64_t)count; ++k) words[k] = 16ull * nb16;
}

}  // namespace rmq
