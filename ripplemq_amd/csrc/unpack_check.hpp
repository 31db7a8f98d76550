// unpack_check.hpp — the structure checks and the length clamp of rmq_unpack (FORMAT.md §7 "Record
// columns"), shared by the unpack kernels (unpack.hip) and the host (tools/unpack_check_main.cpp runs
// them under the sanitizers, at positions and record counts past 2^32). Plain C++, 64-bit and
// unsigned throughout; every range is tested by subtraction, so no sum of caller words can wrap.
// A word that passes here is safe to use as an address inside the caller's arrays.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RMQ_UNPACK_HD __host__ __device__ __forceinline__
#else
#define RMQ_UNPACK_HD inline
#endif

namespace rmq {

constexpr int kUnpackOk = 0;  // RMQ_OK

// The records row r owns, from the words of its result row (rmq_fetch_table's rule): count if its
// status is RMQ_OK and count > 0, else none.
RMQ_UNPACK_HD uint64_t unpack_row_records(uint32_t count, int32_t status) { return status == kUnpackOk ? count : 0; }

// The row checks. t0 = rec_row[r], t1 = rec_row[r + 1]; recs = unpack_row_records of the row.
// rec_row non-decreasing and inside rec_words (t1 <= rec_words for every row gives rec_row[n] <=
// rec_words); the row's word count is the table rule's (recs + 1, or 0); an owning row's run is
// 16-byte aligned inside buf[0, buf_bytes) and can hold its records (16 bytes each at least).
RMQ_UNPACK_HD bool unpack_row_ok(uint64_t t0, uint64_t t1, uint64_t rec_words, uint64_t recs, uint64_t out_pos,
                                 uint64_t bytes, uint64_t buf_bytes) {
  if (t0 > t1 || t1 > rec_words) return false;
  if (t1 - t0 != (recs ? recs + 1ull : 0ull)) return false;
  if (!recs) return true;  // no word and no byte of it is used
  if (out_pos & 15ull) return false;
  if (bytes > buf_bytes || out_pos > buf_bytes - bytes) return false;
  return recs <= bytes / 16ull;
}

// The check of table word k of an owning row (k in [0, recs)): w0 = rec_pos[t0 + k], w1 =
// rec_pos[t0 + k + 1]. The words start at 0, are multiples of 16, increase by at least 16 and end at
// the row's bytes; every k passing means the whole row does. A passing word has w0 + 16 <= w1 <= bytes.
RMQ_UNPACK_HD bool unpack_word_ok(uint64_t k, uint64_t recs, uint64_t w0, uint64_t w1, uint64_t bytes) {
  if ((w0 | w1) & 15ull) return false;
  if (k == 0 && w0 != 0) return false;
  if (w1 > bytes || w0 >= w1) return false;  // (multiples of 16: w1 - w0 >= 16)
  return k + 1ull != recs || w1 == bytes;
}

// len[j] of a record whose header holds hdr_len and whose image has `extent` bytes (a multiple of
// 16, >= 16): min(hdr_len, extent - 16); *mismatch: the length word disagrees with the extent.
RMQ_UNPACK_HD uint32_t unpack_len(uint32_t hdr_len, uint64_t extent, bool* mismatch) {
  const uint64_t room = extent - 16ull;
  *mismatch = 16ull + (((uint64_t)hdr_len + 15ull) & ~15ull) != extent;
  return (uint64_t)hdr_len < room ? hdr_len : (uint32_t)(room < 0xFFFFFFFFull ? room : 0xFFFFFFFFull);
}

// The row that owns record j: the r in [0, n) with first(r) <= j < first(r + 1), for first
// non-decreasing over [0, n] with first(0) <= j < first(n). `first` is called with indices in [1, n).
template <typename FirstFn>
RMQ_UNPACK_HD uint32_t unpack_row_of(uint64_t j, uint32_t n, FirstFn first) {
  uint32_t lo = 0, hi = n - 1u;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (first(mid + 1u) <= j) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// Whether R records of `stride` bytes fit in payload_cap (R * stride may not fit in 64 bits).
RMQ_UNPACK_HD bool unpack_strided_fits(uint64_t R, uint32_t stride, uint64_t payload_cap) {
  return !stride || R <= payload_cap / stride;
}

}  // namespace rmq
