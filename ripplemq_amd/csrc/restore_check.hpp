// restore_check.hpp — the host side of rmq_restore that needs no device (FORMAT.md §11 "Host
// checks"): a verdict per item, and the plan of what is staged for the ones that pass. Plain C++
// over host arrays, so that it also builds into a stand-alone program under the sanitizers
// (tools/restore_check_main.cpp).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/ripplemq_engine.h"

namespace rmq {

constexpr uint64_t kRestoreMax = 1ull << 59;  // offsets and positions stay below it (the ack word of §9)

// What the checks need to know of partition p.
struct RestorePart {
  uint64_t seg;      // S_p
  bool pristine;     // log start and end offsets and positions all 0
  bool local;        // this engine holds a replica slot of it
};

struct RestorePlan {
  std::vector<int32_t> status;     // [n] RMQ_OK: accepted
  std::vector<uint32_t> accepted;  // indices of the accepted items, in call order
  std::vector<uint64_t> rbase;     // [accepted + 1] exclusive scan of their record counts
  // the covering spans of the accepted items' runs (bytes of buf) and tables (words of rec_pos):
  // what a host buffer's staging copies; empty spans are {0, 0}
  uint64_t buf_lo = 0, buf_hi = 0, tab_lo = 0, tab_hi = 0;
  uint64_t bytes = 0;              // run bytes of the accepted items
};

// The verdict on one item from its own words and the partition's geometry (no state of the call).
template <typename PartFn>
int32_t restore_check_item(const rmq_restore_item& it, uint32_t P, uint64_t buf_bytes, uint64_t rec_words, PartFn part) {
  if (it.pidx >= P) return RMQ_ENOPART;
  if (it.flags) return RMQ_EINVAL;
  if ((it.first_pos | it.buf_pos | it.bytes) & 15ull) return RMQ_EINVAL;
  if (it.count > it.bytes / 16ull || (it.count == 0 && it.bytes != 0)) return RMQ_EINVAL;
  // ranges by subtraction: no sum of caller words can wrap
  if (it.bytes > buf_bytes || it.buf_pos > buf_bytes - it.bytes) return RMQ_EINVAL;
  if (it.count >= rec_words || it.table_start > rec_words - (it.count + 1ull)) return RMQ_EINVAL;
  if (it.first_offset >= kRestoreMax || it.count >= kRestoreMax - it.first_offset) return RMQ_EINVAL;
  if (it.first_pos >= kRestoreMax || it.bytes >= kRestoreMax - it.first_pos) return RMQ_EINVAL;
  if (it.commit < it.first_offset || it.commit > it.first_offset + it.count) return RMQ_EINVAL;
  const RestorePart g = part(it.pidx);
  if (it.bytes > g.seg) return RMQ_ENOSPC;  // FORMAT.md §10: log_end_pos - log_start_pos <= S_p
  if (!g.pristine || !g.local) return RMQ_EINVAL;
  return RMQ_OK;
}

template <typename PartFn>
RestorePlan restore_plan(uint32_t n, const rmq_restore_item* items, uint32_t P, uint64_t buf_bytes, uint64_t rec_words,
                         PartFn part) {
  RestorePlan pl;
  pl.status.assign(n, RMQ_OK);
  pl.rbase.push_back(0);
  std::vector<uint8_t> seen(P, 0);
  for (uint32_t i = 0; i < n; ++i) {
    const rmq_restore_item& it = items[i];
    int32_t s = restore_check_item(it, P, buf_bytes, rec_words, part);
    if (s == RMQ_OK && seen[it.pidx]) s = RMQ_EINVAL;  // one item per partition and call
    pl.status[i] = s;
    if (s != RMQ_OK) continue;
    seen[it.pidx] = 1;
    const uint64_t t1 = it.table_start + it.count + 1ull;
    if (pl.accepted.empty()) {
      pl.tab_lo = it.table_start, pl.tab_hi = t1;
    } else {
      pl.tab_lo = it.table_start < pl.tab_lo ? it.table_start : pl.tab_lo;
      pl.tab_hi = t1 > pl.tab_hi ? t1 : pl.tab_hi;
    }
    if (it.bytes) {
      if (pl.buf_lo == pl.buf_hi) {
        pl.buf_lo = it.buf_pos, pl.buf_hi = it.buf_pos + it.bytes;
      } else {
        pl.buf_lo = it.buf_pos < pl.buf_lo ? it.buf_pos : pl.buf_lo;
        pl.buf_hi = it.buf_pos + it.bytes > pl.buf_hi ? it.buf_pos + it.bytes : pl.buf_hi;
      }
    }
    pl.accepted.push_back(i);
    pl.rbase.push_back(pl.rbase.back() + it.count);
    pl.bytes += it.bytes;
  }
  return pl;
}

// The return value of the call from its rows: RMQ_OK, or the status of the lowest-index row that is not.
inline int restore_return(const std::vector<int32_t>& status) {
  for (int32_t s : status)
    if (s != RMQ_OK) return s;
  return RMQ_OK;
}

}  // namespace rmq
