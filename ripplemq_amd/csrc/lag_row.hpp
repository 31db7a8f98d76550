// lag_row.hpp — the arithmetic of one rmq_lag row (FORMAT.md §7 "Lag"), shared by the lag kernel
// (fetch.hip) and the host (tools/lag_row_main.cpp checks it against a brute-force restatement).
// Everything is 64-bit and unsigned; no word here is an address.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RMQ_LAG_HD __host__ __device__ __forceinline__
#else
#define RMQ_LAG_HD inline
#endif

namespace rmq {

constexpr uint64_t kLagNone = ~0ull;  // RMQ_OFFSET_NONE
constexpr int kLagOk = 0, kLagOffset = -6;  // RMQ_OK, RMQ_EOFFSET

// What is known of a row that passed the checks before any position is: where a fetch would start,
// how many records lie before `end` (the high watermark), how many retention took.
struct LagPlan {
  uint64_t start_offset, records, evicted;
  int status;
};

// off: where the reader stands; end: the high watermark; log_start: the first retained offset.
RMQ_LAG_HD LagPlan lag_plan(uint64_t off, uint64_t end, uint64_t log_start) {
  LagPlan p{off, 0, 0, kLagOk};
  if (off >= end) return p;  // caught up
  if (off < log_start) {
    p.status = kLagOffset;
    p.start_offset = log_start;
    p.evicted = log_start - off;
  }
  p.records = end > p.start_offset ? end - p.start_offset : 0;  // (a high watermark below the log start: none)
  return p;
}

// Record bytes the partition can still take before retention evicts the record at start_pos
// (FORMAT.md §7 "Lag"): retention evaluated at log end e evicts up to the first index boundary at
// or after e - ring, so the record goes once e - ring exceeds both the log start and the boundary at
// or below it. ring: the partition's ring bytes; interval_log2: log2 of the index interval.
// 0 for a state no log can have (more than `ring` bytes retained).
RMQ_LAG_HD uint64_t lag_headroom(uint64_t start_pos, uint64_t log_start_pos, uint64_t log_end_pos, uint64_t ring,
                                 uint32_t interval_log2) {
  if (log_end_pos < log_start_pos || log_end_pos - log_start_pos > ring) return 0;
  const uint64_t floor_pos = (start_pos >> interval_log2) << interval_log2;
  const uint64_t keep = floor_pos > log_start_pos ? floor_pos : log_start_pos;
  // keep >= log_start_pos >= log_end_pos - ring, so this is not negative
  return keep + ring - log_end_pos;
}

// The row's words from the plan and the positions of records start_offset and `end` (ignored when
// the plan holds no records).
struct LagRow {
  uint64_t start_offset, records, bytes, evicted, start_pos, end_pos, headroom;
  int status;
};

RMQ_LAG_HD LagRow lag_row(const LagPlan& p, uint64_t start_pos, uint64_t end_pos, uint64_t log_start_pos,
                          uint64_t log_end_pos, uint64_t ring, uint32_t interval_log2) {
  LagRow r{p.start_offset, p.records, 0, p.evicted, 0, 0, kLagNone, p.status};
  if (!p.records) return r;
  r.start_pos = start_pos;
  r.end_pos = end_pos;
  r.bytes = end_pos - start_pos;
  r.headroom = lag_headroom(start_pos, log_start_pos, log_end_pos, ring, interval_log2);
  return r;
}

}  // namespace rmq
