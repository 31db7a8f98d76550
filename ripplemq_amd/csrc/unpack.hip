// unpack.hip — fetched records as columns and dense payloads (rmq_unpack, FORMAT.md §7 "Record
// columns"), gfx950.
//
// The input is the answer of a table fetch: a buffer of FORMAT.md §1 record images, the result rows
// and the record table. Five launches follow each other on the pipeline stream; ordering between the
// phases is by launches only (no workgroup waits for another), and every kernel after the first
// reads the control words earlier phases set and returns at once where they say so:
//   rows sum    a thread per row, a workgroup per chunk of kFetchChunk rows: the row checks
//               (unpack_check.hpp), the row's record count into rec_first[r], the chunk's into rsum;
//   rows scan   the same grid: rec_first[r] becomes the records before row r, rec_first[n] = R; the
//               record capacity and the strided payload capacity are judged here;
//   records     a thread per record (a table word, not a row: one row of every record and 16,384
//               rows of ten spread alike), a workgroup per chunk of kUnpackChunk records: the table
//               word checks, the header, the clamped length; the chunk's sum of len into lsum and
//               the mismatched / truncated counts. It writes no column: the packed payload capacity
//               is not judged yet;
//   len scan    one workgroup: lsum becomes its exclusive prefix, the total is judged against
//               payload_cap;
//   emit        the columns and the payload copy. A workgroup takes a chunk of records, a wave a run
//               of 64 of them, a lane per record for the columns; then the wave scans its records'
//               16-byte destination pieces and deals them to its lanes, so the copy is balanced by
//               bytes, not by records. Where the call has fewer chunks than the grid has workgroups,
//               `slices` workgroups share a chunk: slice s takes every slices-th block of 256 pieces
//               of each run (a run of 16-KiB records is 65,536 pieces).
//
// Bounds. A row passes unpack_row_ok before any of its words is an index: its table words lie
// inside rec_pos[0, rec_words), its run inside buf[0, buf_bytes). A record's two table words pass
// unpack_word_ok before the header at out_pos + w0 is loaded: w0 + 16 <= w1 <= bytes. The length
// word is never an address or a loop bound: len is clamped to the extent w1 - w0 - 16, so every
// source piece lies inside the record's own image. Destinations: j < R <= rec_cap for the columns;
// payload_off[j] + len[j] <= sum(len) <= payload_cap (packed), (j + 1) * stride <= R * stride <=
// payload_cap (strided); the emit kernel runs only when no row failed and no capacity is short.
#include "device_common.hpp"
#include "kernels.hpp"
#include "unpack_check.hpp"

namespace rmq {
namespace {

constexpr u32 kUW = kUnpackChunk / 64;  // waves per record workgroup
constexpr u32 kUnroll = 4;              // pieces in flight per lane of the copy
constexpr u32 kMaxSlices = 256;         // workgroups that may share one chunk's copy

struct UnpackRow {
  u64 out_pos, recs;
  u32 bytes;
};
__device__ __forceinline__ UnpackRow load_row(const UnpackArgs& a, u32 r) {
  const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(a.rows + 4ull * r);
  const ulonglong2 hi = *reinterpret_cast<const ulonglong2*>(a.rows + 4ull * r + 2);
  return UnpackRow{lo.y, unpack_row_records((u32)hi.x, (int32_t)(u32)hi.y), (u32)(hi.x >> 32)};
}

__device__ __forceinline__ void flag_bad_row(const UnpackArgs& a, u32 r) {
  atomicMax((unsigned long long*)&a.ctl[kUnpackBad], (unsigned long long)(a.n - r));
}

// Sum of a value over the workgroup's four waves, in every thread (one barrier).
__device__ __forceinline__ u64 wg_sum(u64 v, u64* s_sum) {
  const u64 inc = wave_incl_scan(v);
  if (lane_id() == 63) s_sum[threadIdx.x >> 6] = inc;
  __syncthreads();
  return s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

}  // namespace

// Rows, first half (the shape of fetch_table_sum_kernel).
__global__ __launch_bounds__(kFetchChunk) void unpack_rows_sum_kernel(UnpackArgs a) {
  static_assert(kFetchChunk == 256, "four waves, a thread per row of the chunk");
  const u32 c = blockIdx.x, r = c * kFetchChunk + threadIdx.x;
  __shared__ u64 s_sum[kFetchChunk / 64];
  u64 recs = 0;
  if (r < a.n) {
    const UnpackRow w = load_row(a, r);
    if (unpack_row_ok(a.rec_row[r], a.rec_row[r + 1ull], a.rec_words, w.recs, w.out_pos, w.bytes, a.buf_bytes))
      recs = w.recs;
    else
      flag_bad_row(a, r);
    a.rec_first[r] = recs;
  }
  const u64 sum = wg_sum(recs, s_sum);
  if (threadIdx.x == 0) a.rsum[c] = sum;
}

// Rows, second half (the shape of fetch_table_rows_kernel): rec_first in place, R and the capacity
// verdicts that need R alone.
__global__ __launch_bounds__(kFetchChunk) void unpack_rows_scan_kernel(UnpackArgs a) {
  const u32 c = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  __shared__ u64 s_sum[kFetchChunk / 64];
  if (a.ctl[kUnpackBad]) return;
  u64 base = 0;
  for (u32 k = lane; k < c; k += 64) base += a.rsum[k];
  base = bcast_u64(wave_incl_scan(base), 63);
  const u32 r = c * kFetchChunk + tid;
  const u64 v = r < a.n ? a.rec_first[r] : 0ull;
  const u64 inc = wave_incl_scan(v);
  if (lane == 63) s_sum[w] = inc;
  __syncthreads();
  u64 P = base + inc - v;
  for (u32 k = 0; k < w; ++k) P += s_sum[k];
  if (r < a.n) a.rec_first[r] = P;
  if (r + 1 == a.n) {
    const u64 R = P + v;
    a.rec_first[a.n] = R;
    a.ctl[kUnpackRecords] = R;
    bool stop = R > a.rec_cap;
    if (a.mode == kUnpackStrided) {
      const bool fits = unpack_strided_fits(R, a.stride, ~0ull);
      a.ctl[kUnpackBytes] = fits ? R * a.stride : ~0ull;
      stop = stop || !unpack_strided_fits(R, a.stride, a.payload_cap);
    }
    if (stop) a.ctl[kUnpackStop] = 1;
  }
}

namespace {

// Record j of the call, everything checked: the row that owns it, its image and its clamped length.
struct UnpackRec {
  u32 r, len;
  u64 img;     // byte offset of the header in buf
  u64 offset;  // the header's offset word
  bool ok, mismatch;
};
__device__ __forceinline__ UnpackRec unpack_rec(const UnpackArgs& a, u64 j) {
  UnpackRec q{};
  q.r = unpack_row_of(j, a.n, [&](u32 i) { return a.rec_first[i]; });
  const UnpackRow w = load_row(a, q.r);
  const u64 k = j - a.rec_first[q.r];
  const u64 t = a.rec_row[q.r] + k;
  // (the row passed unpack_row_ok and k < recs: t + 1 < rec_row[r + 1] <= rec_words)
  const u64 w0 = a.rec_pos[t], w1 = a.rec_pos[t + 1ull];
  q.ok = k < w.recs && unpack_word_ok(k, w.recs, w0, w1, w.bytes);
  if (!q.ok) return q;
  q.img = w.out_pos + w0;
  const uint4 h = *reinterpret_cast<const uint4*>(a.buf + q.img);
  q.offset = ((u64)h.y << 32) | h.x;
  q.len = unpack_len(h.z, w1 - w0, &q.mismatch);
  return q;
}

}  // namespace

// Records: the checks and the sums; no column is written.
__global__ __launch_bounds__(kUnpackChunk) void unpack_records_kernel(UnpackArgs a) {
  __shared__ u64 s_sum[kUW];
  if (a.ctl[kUnpackBad]) return;
  const u64 R = a.ctl[kUnpackRecords];
  const u64 chunks = (R + kUnpackChunk - 1ull) / kUnpackChunk;
  for (u64 c = blockIdx.x; c < chunks; c += gridDim.x) {
    const u64 j = c * kUnpackChunk + threadIdx.x;
    u64 len = 0, mis = 0, trunc = 0;
    if (j < R) {
      const UnpackRec q = unpack_rec(a, j);
      if (q.ok) {
        len = q.len;
        mis = q.mismatch;
        trunc = a.mode == kUnpackStrided && q.len > a.stride;
      } else {
        flag_bad_row(a, q.r);
      }
    }
    // one sum for the three: len < 2^32 a record and 256 records a chunk, so 40 bits; 12 bits each for the counts
    const u64 sum = wg_sum(len | (mis << 40) | (trunc << 52), s_sum);
    if (threadIdx.x == 0) {
      a.lsum[c] = sum & ((1ull << 40) - 1ull);
      if ((sum >> 40) & 0xFFFull) atomicAdd((unsigned long long*)&a.ctl[kUnpackMismatch], (unsigned long long)((sum >> 40) & 0xFFFull));
      if (sum >> 52) atomicAdd((unsigned long long*)&a.ctl[kUnpackTrunc], (unsigned long long)(sum >> 52));
    }
    __syncthreads();  // s_sum is read before the next round writes it
  }
}

// Len scan: one workgroup turns the chunk sums into their exclusive prefix and judges the packed
// payload capacity.
__global__ __launch_bounds__(kUnpackChunk) void unpack_len_scan_kernel(UnpackArgs a) {
  __shared__ u64 s_sum[kUW];
  if (a.ctl[kUnpackBad]) return;
  const u32 tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const u64 R = a.ctl[kUnpackRecords];
  const u64 chunks = (R + kUnpackChunk - 1ull) / kUnpackChunk;
  u64 carry = 0;
  for (u64 c0 = 0; c0 < chunks; c0 += kUnpackChunk) {
    const u64 c = c0 + tid;
    const u64 v = c < chunks ? a.lsum[c] : 0ull;
    const u64 inc = wave_incl_scan(v);
    if (lane == 63) s_sum[w] = inc;
    __syncthreads();
    u64 P = carry + inc - v;
    for (u32 k = 0; k < w; ++k) P += s_sum[k];
    if (c < chunks) a.lsum[c] = P;
    carry += s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    __syncthreads();
  }
  if (tid == 0 && a.mode == kUnpackPacked) {
    a.ctl[kUnpackBytes] = carry;
    if (carry > a.payload_cap) a.ctl[kUnpackStop] = 1;
  }
}

namespace {

typedef u32x4 __attribute__((aligned(1))) u32x4_u;
typedef u64 __attribute__((aligned(1))) u64_u;
typedef u32 __attribute__((aligned(1))) u32_u;
typedef uint16_t __attribute__((aligned(1))) u16_u;

// The first nb (1..16) bytes of v to dst, at any byte alignment.
__device__ __forceinline__ void store_bytes(uint8_t* dst, uint4 v, u32 nb) {
  if (nb >= 16u) {
    const u32x4 x = {v.x, v.y, v.z, v.w};
    *reinterpret_cast<u32x4_u*>(dst) = x;
    return;
  }
  u64 lo = ((u64)v.y << 32) | v.x;
  if (nb & 8u) {
    *reinterpret_cast<u64_u*>(dst) = lo;
    dst += 8;
    lo = ((u64)v.w << 32) | v.z;
  }
  if (nb & 4u) {
    *reinterpret_cast<u32_u*>(dst) = (u32)lo;
    dst += 4;
    lo >>= 32;
  }
  if (nb & 2u) {
    *reinterpret_cast<u16_u*>(dst) = (uint16_t)lo;
    dst += 2;
    lo >>= 16;
  }
  if (nb & 1u) *dst = (uint8_t)lo;
}

// v with every byte from nv (0..15) on set to zero.
__device__ __forceinline__ uint4 keep_bytes(uint4 v, u32 nv) {
  u64 lo = ((u64)v.y << 32) | v.x, hi = ((u64)v.w << 32) | v.z;
  if (nv < 8u) {
    hi = 0;
    lo &= (1ull << (8u * nv)) - 1ull;
  } else {
    hi &= (1ull << (8u * (nv - 8u))) - 1ull;
  }
  return make_uint4((u32)lo, (u32)(lo >> 32), (u32)hi, (u32)(hi >> 32));
}

}  // namespace

// Emit: the columns, then the copy.
__global__ __launch_bounds__(kUnpackChunk) void unpack_emit_kernel(UnpackArgs a) {
  __shared__ u64 s_sum[kUW];
  __shared__ u64 s_end[kUW][64];   // inclusive scan of the run's destination pieces
  __shared__ u64 s_src[kUW][64];   // payload's byte offset in buf
  __shared__ u64 s_dst[kUW][64];   // its byte offset in the payload area
  __shared__ u32 s_dlen[kUW][64];  // destination bytes (packed: len; strided: stride)
  __shared__ u32 s_clen[kUW][64];  // bytes copied (strided: min(len, stride); zero behind them)
  if (a.ctl[kUnpackBad] | a.ctl[kUnpackStop]) return;
  const u32 tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const u64 R = a.ctl[kUnpackRecords];
  const u64 chunks = (R + kUnpackChunk - 1ull) / kUnpackChunk;
  if (!chunks) return;
  // workgroups that share a chunk's copy (view mode copies nothing)
  const u64 per = gridDim.x / chunks;
  const u32 slices = a.mode == kUnpackView || per < 1ull ? 1u : per > kMaxSlices ? kMaxSlices : (u32)per;
  for (u64 u = blockIdx.x; u < chunks * slices; u += gridDim.x) {
    const u64 c = u / slices;
    const u32 s = (u32)(u % slices);
    const u64 j = c * kUnpackChunk + tid;
    UnpackRec q{};
    if (j < R) q = unpack_rec(a, j);
    const bool live = j < R && q.ok;  // (every record passed in the records kernel; a word changed since is skipped)
    const u64 src = q.img + 16ull;
    u32 len = live ? q.len : 0u;
    u64 dst = 0;
    if (a.mode == kUnpackPacked) {  // the chunk's base, the waves before this one, the lanes before this one
      const u64 inc = wave_incl_scan((u64)len);
      if (lane == 63) s_sum[w] = inc;
      __syncthreads();
      dst = a.lsum[c] + inc - len;
      for (u32 k = 0; k < w; ++k) dst += s_sum[k];
    } else if (a.mode == kUnpackStrided) {
      dst = j * a.stride;
    }
    if (live && s == 0) {
      if (a.offset) a.offset[j] = q.offset;
      a.len[j] = len;
      a.payload_off[j] = a.mode == kUnpackView ? src : dst;
      if (a.tag) a.tag[j] = a.row_tag ? a.row_tag[q.r] : q.r;
    }
    if (a.mode != kUnpackView) {
      const u32 dlen = !live ? 0u : a.mode == kUnpackStrided ? a.stride : len;
      const u32 clen = len < dlen ? len : dlen;
      const u64 pieces = ((u64)dlen + 15ull) >> 4;
      const u64 end = wave_incl_scan(pieces);
      s_end[w][lane] = end, s_src[w][lane] = src, s_dst[w][lane] = dst, s_dlen[w][lane] = dlen, s_clen[w][lane] = clen;
      // (the wave's own rows of LDS: written and read by the same wave, in program order)
      __builtin_amdgcn_wave_barrier();
      const u64 T = bcast_u64(end, 63);
      const u64 step = 64ull * kUnroll;
      for (u64 q0 = (u64)s * step; q0 < T; q0 += (u64)slices * step) {
        uint4 v[kUnroll];
        uint8_t* d[kUnroll];
        u32 nb[kUnroll];
#pragma unroll
        for (u32 x = 0; x < kUnroll; ++x) {
          const u64 p = q0 + 64ull * x + lane;
          nb[x] = 0;
          v[x] = make_uint4(0, 0, 0, 0);
          if (p < T) {
            u32 lo = 0, hi = 63;  // the first record whose pieces end beyond p
            while (lo < hi) {
              const u32 mid = (lo + hi) >> 1;
              if (s_end[w][mid] <= p) lo = mid + 1u; else hi = mid;
            }
            const u32 dl = s_dlen[w][lo], cl = s_clen[w][lo];
            const u64 m16 = 16ull * (p - (s_end[w][lo] - (((u64)dl + 15ull) >> 4)));  // the piece's byte offset in its record
            const u64 left = (u64)dl - m16;
            nb[x] = left < 16ull ? (u32)left : 16u;
            d[x] = a.payload + s_dst[w][lo] + m16;
            if (m16 < cl) {
              v[x] = load_payload16(a.buf + s_src[w][lo] + m16);
              if ((u64)cl - m16 < 16ull) v[x] = keep_bytes(v[x], (u32)((u64)cl - m16));
            }
          }
        }
#pragma unroll
        for (u32 x = 0; x < kUnroll; ++x)
          if (nb[x]) store_bytes(d[x], v[x], nb[x]);
      }
    }
    __syncthreads();  // s_sum is read before the next round writes it
  }
}

void launch_unpack(const UnpackArgs& a, uint32_t max_wgs, hipStream_t s) {
  if (!a.n) return;
  const dim3 chunks((a.n + kFetchChunk - 1) / kFetchChunk);
  hipLaunchKernelGGL(unpack_rows_sum_kernel, chunks, dim3(kFetchChunk), 0, s, a);
  hipLaunchKernelGGL(unpack_rows_scan_kernel, chunks, dim3(kFetchChunk), 0, s, a);
  // R is at most the table's words: the record grids cover what rec_words allows, capped
  const uint64_t rc = a.rec_words / kUnpackChunk + 1;
  const uint32_t cap = std::max<uint32_t>(max_wgs, 1u);
  const uint32_t wgs = (uint32_t)std::min<uint64_t>(rc, cap);
  hipLaunchKernelGGL(unpack_records_kernel, dim3(wgs), dim3(kUnpackChunk), 0, s, a);
  hipLaunchKernelGGL(unpack_len_scan_kernel, dim3(1), dim3(kUnpackChunk), 0, s, a);
  if (!a.rec_cap) return;  // a size probe
  // the emit grid is the cap itself: workgroups beyond the chunks share the chunks' copies
  hipLaunchKernelGGL(unpack_emit_kernel, dim3(a.mode == kUnpackView ? wgs : cap), dim3(kUnpackChunk), 0, s, a);
}

}  // namespace rmq
