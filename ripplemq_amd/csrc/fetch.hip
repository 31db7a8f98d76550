// fetch.hip — batched consumer fetch: PartitionStateMachine.handleBatchRead
// (mq-broker/src/main/java/metadata/raft/PartitionStateMachine.java:85-110), served directly from
// committed state like MessageBatchReadRequestProcessor.java:39 (no read-index).
//
//  resolve (half-wave per request, two per wave: 16,384 requests are 8,192 waves, about one round
//          of the chip's resident waves): off = consumerOffsets.getOrDefault(id, 0); end = min(off + max, hw);
//          byte range of records [off, end): both ends found together, a quarter-wave each, by a
//          16-ary search of the sparse offset index (FORMAT.md §5: E[m] = first record starting at
//          or after m*I; 16 probes per round, one round per factor 16 of index entries), then the
//          record headers of the 512 B after the entry found are loaded at once (two 16-byte pieces
//          per lane of the quarter) and walked in registers;
//          each workgroup adds its requests' bytes to the sum of their chunk of 256 requests;
//  gather  (workgroup per 16 requests, a wave per 4): the output position of its first request from
//          the chunk sums before it and the byte counts of its chunk before it (at most 64 + 255
//          values, L2-resident), an exclusive scan over its 16 requests -> compact output positions
//          (into the result rows' out_pos), ENOSPC marking (every request's bytes count, served or
//          not: FORMAT.md §7); then each wave copies its 4 requests one after the other (the
//          requests' ring words loaded before the placement barrier), 16-byte loads from the
//          lowest local replica ring, four in flight per lane, 16-byte stores to the output. Records and output positions are 16-byte aligned
//          (FORMAT.md §1), so no piece straddles a record, the ring end or an output boundary.
//          (Round 2 placed with a single 1024-thread workgroup between the two: 12.6 us of the
//          max = 10 fetch of 16,384 requests with the rest of the GPU idle.)
//  trim    (only a ticket with byte budgets, rmq_fetch_bytes; between the two; a quarter-wave per
//          request): a served request whose bytes exceed its budget is cut at the last record
//          start inside the budget, found from the position-keyed sparse index and a walk of the
//          length words up to the limit, and the words the gather places and copies from are
//          rewritten.
//  fill    (only a ticket with RMQ_FETCH_FILL; before the gather; a workgroup per chunk of 256
//          requests): out_cap bounds the whole call: a prefix scan over the requests' bytes finds
//          the request that crosses the end of the output, which is cut by the trim's own search
//          and walk; the served requests after it are put off (RMQ_PENDING).
//  lag     (rmq_lag, a call of its own; the resolve's shape and its search): per row the records and
//          bytes between the reader and the high watermark and the partition's retention headroom;
//          writes nothing of the engine.
//
// The kernels (resolve, gather; the chunk sums a slot's previous gather cleared) run on the
// pipeline stream itself, after the last pipeline launch the host had issued and before the next
// one, so the committed state they read is stable and the append pipeline is never flushed for a
// fetch.
#include <hip/hip_ext.h>

#include <algorithm>
#include <type_traits>

#include "device_common.hpp"
#include "fetch_table_walk.hpp"
#include "kernels.hpp"
#include "lag_row.hpp"

namespace rmq {

constexpr int kOk = 0, kNotLeader = -1, kNoPart = -2, kInval = -3, kNoSpc = -4, kOffset = -6;
constexpr u32 kFW = 4;  // waves per workgroup (gather)
#ifndef RMQ_RESOLVE_WAVES
#define RMQ_RESOLVE_WAVES 8  // round 5 (rows read by one load per workgroup): 8 vs 4 waves, max = 10
                             // 24.8-25.3 vs 25.1-25.5 us, consumer loop 36.0 vs 36.9-37.6 us; 16: max = 10 27 us
#endif
constexpr u32 kRW = RMQ_RESOLVE_WAVES;  // waves per resolve workgroup

struct PartView {
  u64 leo, used, start_off, start_pos;
  RingRef rg;           // the partition's ring and index ring
  const uint8_t* ring;  // lowest local replica ring of the partition
};

// A wave resolves two requests (lanes 0..31 and 32..63), and each request's two ends are found
// together by a quarter-wave each: kQL lanes per searched position.
constexpr u32 kQL = 16;
constexpr u64 kWalkMax = 32;  // longest slice walked from a cached position
constexpr u32 kRPW = 2;  // requests per resolve wave

// Logical byte position of record t (start_off <= t <= leo) in the lane's view, found by the kQL
// lanes of its quarter (t, v, act quarter-uniform; an inactive quarter loads nothing and gets 0).
// The largest index entry at or before t: E[m] = first record starting at or after m I rises with
// m, so a kQL-ary search over the live entries (round 0 probes the kQL entries around the
// interpolated position of t: records of one size give it exactly), then the record headers after
// that entry, read as windows of 2 kQL 16-byte pieces (two per lane) and walked in registers; the
// window the interpolation puts t in is loaded with the first probe round and used when the entry
// found lies inside it.
#ifndef RMQ_FETCH_PPL
#define RMQ_FETCH_PPL 2
#endif
// header-window pieces per lane: 2 (512 B windows); 4 (1 KB: the whole 1 KB interval in one window)
// measured slower, 28.1-29.1 vs 26.5-26.8 us per max = 10 fetch (more loads, 6 waves per SIMD)
constexpr u32 kPPL = RMQ_FETCH_PPL;
static_assert(kPPL == 2 || kPPL == 4, "two or four pieces per lane");

// The length words of window pieces kPPL*hl .. kPPL*hl + kPPL-1 (16-byte pieces from byte wb).
struct WinWords {
  u32 w[4];
};
__device__ __forceinline__ WinWords load_window(const uint8_t* ring, u64 wb, u32 hl, u64 mask) {
  WinWords x{};
#pragma unroll
  for (u32 k = 0; k < kPPL; ++k)
    x.w[k] = *reinterpret_cast<const u32*>(ring + ((wb + 16ull * (kPPL * hl + k) + 8ull) & mask));
  return x;
}

// hit: the position cache holds the position of record h_off <= t (h_pos): no index search, the
// walk starts there.
__device__ __forceinline__ u64 record_posq(const DevState& st, const PartView& v, u64 t, bool act, bool hit,
                                           u64 h_off, u64 h_pos) {
  const u32 lane = lane_id(), h = lane / kQL, hl = lane % kQL;
  constexpr u32 kWin = kPPL * kQL;  // pieces per header window
  const u32 ilog = st.interval_log2;
  const u64 I = 1ull << ilog;
  const u64* E = st.index + v.rg.ibase * 2;
  u64 c_off = v.start_off, c_pos = v.start_pos;
  long lo = (long)((v.start_pos + I - 1) >> ilog), hi = (long)(v.used >> ilog);
  bool open = act && t < v.leo && lo <= hi;
  long ws = lo, step = 1;
  const u64 mask = v.rg.seg - 1;
  u64 sw = ~0ull;  // speculative header window
  if (act && hit) {
    open = false;
    c_off = h_off;
    c_pos = h_pos;
    sw = h_pos & ~15ull;
  } else if (open) {
    const double f = (double)(t - v.start_off) / (double)(v.leo - v.start_off);
    const u64 gpos = v.start_pos + (u64)(f * (double)(v.used - v.start_pos));
    const long me = (long)(gpos >> ilog);
    ws = max(lo, min(me - (long)(kQL / 2 - 1), hi - (long)(kQL - 1)));
    sw = max((u64)me << ilog, v.start_pos) & ~15ull;
  } else if (act && t < v.leo) {
    sw = v.start_pos;  // no index entry past the start: the walk starts at the log start
  }
  WinWords Sw{};
  if (sw != ~0ull) Sw = load_window(v.ring, sw, hl, mask);
  constexpr u32 kQMask = (1u << kQL) - 1u;
  for (bool first = true; __any(open); first = false) {
    if (!first) {
      ws = lo;
      step = (hi - lo + (long)kQL) / (long)kQL;
    }
    const long we = min(hi, ws + (long)(kQL - 1) * step);  // last probe of the round
    const long m = ws + (long)hl * step;
    bool le = false;
    u64 eo = 0, ep = 0;
    if (open && m <= we) {
      const u64* e = E + ((u64)m % v.rg.icap) * 2;
      eo = e[0];
      ep = e[1];
      le = eo <= t;
    }
    const u32 bal = (u32)(__ballot(le) >> (kQL * h)) & kQMask;  // this quarter's probes
    const u32 last = bal ? 31u - (u32)__builtin_clz(bal) : 0u;
    const u64 so = __shfl(eo, (int)(kQL * h + last), 64), sp = __shfl(ep, (int)(kQL * h + last), 64);
    if (open) {
      if (!bal) {  // every probe past t: the answer precedes this round's first probe
        hi = ws - 1;
        open = lo <= hi;
      } else {
        c_off = so;
        c_pos = sp;
        const long mk = ws + (long)last * step;  // a probe at or before t
        if (step == 1 && (mk < we || we == hi)) {
          open = false;  // the next entry is past t (or there is none)
        } else {
          lo = mk + 1;  // the answer is that probe or a later entry, up to the next probe
          if (step > 1 && mk < we) hi = min(hi, mk + step - 1);
          open = lo <= hi;
        }
      }
    }
  }
  if (!act) return 0;
  if (t >= v.leo) return v.used;
  u64 wb = sw;
  WinWords Lw = Sw;
  u32 cur = (u32)((c_pos - sw) >> 4);  // window piece of the current record
  if (sw == ~0ull || c_pos < sw || c_pos >= sw + 16ull * kWin) {
    wb = c_pos;
    cur = 0;
    Lw = load_window(v.ring, wb, hl, mask);
  }
  u64 k = t - c_off;
  while (__any(k > 0)) {
    const bool mv = k > 0 && cur >= kWin;  // quarter-uniform: the quarter walked off its window
    if (__any(mv)) {
      if (mv) {
        wb += 16ull * cur;
        cur = 0;
        Lw = load_window(v.ring, wb, hl, mask);
      }
    }
    const u32 src = kQL * h + (cur / kPPL);
    u32 a = 0;
#pragma unroll
    for (u32 q = 0; q < kPPL; ++q) {
      const u32 x = (u32)__shfl((int)Lw.w[q], (int)(src & 63u), 64);
      a = (cur % kPPL) == q ? x : a;
    }
    if (k > 0) {
      cur += record_bytes(a) >> 4;
      --k;
    }
  }
  return wb + 16ull * cur;
}

// Request r, resolved by one half-wave (half-uniform results): status, start offset, count,
// bytes, the source position and the ring word {ring byte offset in logs << 6 | log2(ring bytes)}.
struct Resolved {
  u64 start, count, bytes, pos0, ring;
  int status;
};

// kAt (rmq_fetch_at, FORMAT.md §7 "Explicit offsets"): `at` is the request's explicit offset, or
// RMQ_OFFSET_NONE for the table's; it replaces the table word once that has been loaded (the load
// stays in the round of the partition's other words) and nothing after `off` knows the difference.
template <bool kAt>
__device__ __forceinline__ Resolved resolve_request(const FetchArgs& a, const uint4 rq, bool live, u64 at) {
  const DevState& st = a.st;
  const u32 p = rq.x, c = rq.y, mx = rq.z;
  int status = kOk;
  u64 start = 0, count = 0, end = 0, ring_off = 0;
  // every word of the partition in one round, the leader flag included (a request refused by the
  // checks below, or with an empty slice, leaves them unused)
  const bool okp = live && p < st.P;
  const u32 pp = okp ? p : 0u, cc = c < st.C ? c : 0u;
  const u32 lead = okp ? st.is_leader[pp] : 0u;
  // RMQ_FETCH_REPLICA: this engine's own replica, from its replica cursor, leader or follower
  const bool rep = a.replica && (rq.w & kFetchReplica);
  const u64 tab = okp ? (rep ? st.rcur[pp] : st.cons[(u64)pp * st.C + cc]) : 0ull;
  const u64 hw = okp ? st.hw[pp] : 0ull;
  PartView v;
  v.leo = okp ? st.leo[pp] : 0ull;
  v.used = okp ? st.used[pp] : 0ull;
  v.start_off = okp ? st.start_off[pp] : 0ull;
  v.start_pos = okp ? st.start_pos[pp] : 0ull;
  const u32 lm = okp ? st.local_mask[pp] : 0u;
  const u64 desc = okp ? st.ring[pp] : 0ull;
  const ulonglong2 ce = okp ? *reinterpret_cast<const ulonglong2*>(st.pcache + ((u64)pp * st.C + cc) * 2)
                            : make_ulonglong2(~0ull, 0ull);
  const u64 h_off = ce.x, h_pos = ce.y;
  const u64 off = kAt && okp && at != ~0ull ? at : tab;
  v.rg = ring_ref(desc, st.interval_log2, st.icap_mul);
  v.ring = st.logs;
  bool need = false;  // the slice is not empty: both its ends are searched
  if (!live) {
  } else if (p >= st.P) {
    status = kNoPart;
  } else if (!lead && !rep) {
    status = kNotLeader;
  } else if (c >= st.C) {
    status = kInval;
  } else {
    start = off;
    u64 lim = off + mx;
    if (lim < off) lim = ~0ull;
    end = lim < hw ? lim : hw;
    if (off < end) {
      if (off < v.start_off) {
        status = kOffset;
        start = v.start_off;  // where the consumer can resume (FORMAT.md §7)
      } else {
        const u32 r0 = lm ? (u32)__ffs(lm) - 1u : 0u;
        ring_off = (u64)r0 * st.rstride + v.rg.base;
        v.ring = st.logs + ring_off;
        count = end - off;
        need = true;
      }
    }
  }
  // quarter 0 of the half: the slice's first record, quarter 1: one past its last
  const u32 hb = lane_id() & 32u;
  // the position cache (the record after this consumer's last served slice): a consumer reading on
  // from there skips the index search, and walks from the cached position (a short slice only:
  // a long one takes the search, which skips most of it)
  const bool hit = need && h_off == off && h_pos >= v.start_pos && h_pos < v.used && count <= kWalkMax;
  const u64 pq = record_posq(st, v, (lane_id() & 16u) ? end : off, need, hit, off, h_pos);
  const u64 pos0 = __shfl(pq, (int)hb, 64), pend = __shfl(pq, (int)(hb + 16u), 64);
  return Resolved{start, count, need ? pend - pos0 : 0ull, pos0, (ring_off << 6) | (desc & 63ull), status};
}

// The ticket of workgroup b (wg0: first workgroup of each ticket) and b's index inside it; the
// arguments are read in place from the kernarg segment (an indexed by-value copy could go to scratch).
// kMulti false: a launch of one ticket (every synchronous fetch, every fetch that commits): its
// arguments at fixed kernarg offsets, as before batches existed.
template <bool kMulti>
__device__ __forceinline__ const FetchArgs& ticket_of(const u32* wg0, u32& b) {
  if (!kMulti) return *(const FetchArgs*)__builtin_amdgcn_kernarg_segment_ptr();
  const FetchBatch& B = *(const FetchBatch*)__builtin_amdgcn_kernarg_segment_ptr();
  u32 k = 0;
#pragma unroll
  for (u32 i = 1; i < kFetchBatch; ++i) k += (i < B.nt && b >= wg0[i]) ? 1u : 0u;
  b -= wg0[k];
  return B.t[k];
}

template <bool kMulti>
using FetchKArgs = typename std::conditional<kMulti, FetchBatch, FetchArgs>::type;  // (t[0] first in both)
static_assert(offsetof(FetchBatch, t) == 0, "a batch's first ticket at the kernarg base");

// kAt: the single-ticket instantiation of a call with explicit offsets (a.at != null); the other
// two never look at a.at.
template <bool kMulti, bool kAt = false>
__global__ __launch_bounds__(64 * kRW) void fetch_resolve_kernel(FetchKArgs<kMulti> batch) {
  static_assert(!(kMulti && kAt), "a ticket with explicit offsets is launched alone");
  (void)batch;
  const FetchBatch& B = *(const FetchBatch*)__builtin_amdgcn_kernarg_segment_ptr();
  u32 bid = blockIdx.x;
  const FetchArgs& a = ticket_of<kMulti>(B.rwg0, bid);
  const u32 lane = lane_id(), w = threadIdx.x >> 6;
  const u32 r = (bid * kRW + w) * kRPW + (lane >> 5);
  const bool live = r < a.n;  // (no early return: the workgroup meets at barriers below)
  // the workgroup's request rows, read once by one load of consecutive 16-byte rows (host rows:
  // one PCIe read of 128 bytes instead of a 16-byte read per request), through LDS; the device
  // copy for the gather and the position cache
  __shared__ uint4 s_rq[kRW * kRPW];
  // (kAt) and their explicit offsets beside them, by one load of consecutive 8-byte words (host
  // rows: one more PCIe read of 128 bytes, in flight with the rows')
  __shared__ u64 s_at[kAt ? kRW * kRPW : 1];
  {
    const u32 r0 = bid * kRW * kRPW + threadIdx.x;
    if (threadIdx.x < kRW * kRPW && r0 < a.n) {
      const uint4 x = *reinterpret_cast<const uint4*>(a.req + 4ull * r0);
      if (kAt) s_at[threadIdx.x] = a.at[r0];
      s_rq[threadIdx.x] = x;
      if (a.req != a.req_dev) *reinterpret_cast<uint4*>(a.req_dev + 4ull * r0) = x;
    }
  }
  __syncthreads();
  const Resolved q = resolve_request<kAt>(a, live ? s_rq[w * kRPW + (lane >> 5)] : make_uint4(0, 0, 0, 0), live,
                                          kAt && live ? s_at[w * kRPW + (lane >> 5)] : ~0ull);
  __shared__ u64 s_b[kRW];
  const u64 b2 = bcast_u64(q.bytes, 0) + bcast_u64(q.bytes, 32);  // the wave's two requests
  if (lane == 0) s_b[w] = b2;
  if (live && (lane & 31u) == 0) {
    // the position cache's next entry for this consumer: the record after the slice (a served
    // request's partition and consumer are in range; reloaded here rather than held through the
    // resolve, which would take 8 more VGPRs)
    if (q.status == kOk && q.count) {
      // one 16-byte store: requests of one (partition, consumer) in one call (allowed when none
      // commits) each write a true {offset, position} pair, and a pair is never torn between two
      u64* ce = a.st.pcache + ((u64)a.req_dev[4 * r] * a.st.C + a.req_dev[4 * r + 1]) * 2;
      *reinterpret_cast<ulonglong2*>(ce) = make_ulonglong2(q.start + q.count, q.pos0 + q.bytes);
    }
    a.res[4 * r + 0] = q.start;
    a.res[4 * r + 2] = q.count | (q.bytes << 32);
    a.res[4 * r + 3] = (u64)(uint32_t)q.status;
    a.aux[2 * r + 0] = q.pos0;
    a.aux[2 * r + 1] = q.ring;
    a.cpre[r] = (u32)q.bytes;
  }
  // one add per workgroup (its kRW * kRPW requests share a chunk) into the chunk's own L2 line
  static_assert(kFetchChunk % (kRW * kRPW) == 0, "a resolve workgroup never straddles a chunk");
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 b = 0;
    for (u32 k = 0; k < kRW; ++k) b += s_b[k];
    if (b) atomicAdd((unsigned long long*)&a.csum[(u64)(bid * kRW * kRPW / kFetchChunk) * kCsumStride], (unsigned long long)b);
  }
}

// Lane src's value (src per lane).
__device__ __forceinline__ u64 shfl_u64(u64 v, int src) {
  return ((u64)(u32)__shfl((int)(v >> 32), src, 64) << 32) | (u32)__shfl((int)(u32)v, src, 64);
}

constexpr u32 kGQ = 4;          // requests per gather wave
constexpr u32 kGR = kFW * kGQ;  // requests per gather workgroup

// Placement + gather: workgroup per kGR consecutive requests. Two rounds of loads: the wave's
// request words with the placement sums, then (requests of at most 128 pieces) the records' pieces,
// issued before the placement barriers; only the stores wait for the output positions.
template <bool kMulti>
__global__ __launch_bounds__(64 * kFW) void fetch_gather_kernel(FetchKArgs<kMulti> batch) {
  (void)batch;
  const FetchBatch& B = *(const FetchBatch*)__builtin_amdgcn_kernarg_segment_ptr();
  u32 bid = blockIdx.x;
  const FetchArgs& a = ticket_of<kMulti>(B.gwg0, bid);
  const u32 nwg = (a.n + kGR - 1) / kGR;  // the ticket's gather workgroups
  __shared__ u64 s_red[kFW];
  __shared__ u64 s_pos[kGR];
  const DevState& st = a.st;
  const u32 tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  const u32 r0 = bid * kGR, c0 = r0 / kFetchChunk;
  // the wave's kGQ requests (lanes 0..kGQ-1 read one each)
  const u32 rq = r0 + w * kGQ + (lane < kGQ ? lane : 0u);
  const bool qv = lane < kGQ && rq < a.n;
  const u64 q_pos = qv ? a.aux[2 * rq + 0] : 0ull, q_ring = qv ? a.aux[2 * rq + 1] : 0ull;
  const u64 q_nb = qv ? a.cpre[rq] : 0ull;
  // the next fetch's chunk sums (its resolve runs after this kernel on the same stream)
  for (u32 k = bid * 64 * kFW + tid; k < a.csum_lines; k += nwg * 64 * kFW) a.csum_next[(u64)k * kCsumStride] = 0;
  // bytes of every request before r0: the chunk sums before its chunk, then its chunk's requests
  u64 v = 0;
  for (u32 k = tid; k < c0; k += 64 * kFW) v += a.csum[(u64)k * kCsumStride];
  for (u32 k = c0 * kFetchChunk + tid; k < r0; k += 64 * kFW) v += a.cpre[k];
  const u32 rr = r0 + tid;
  const u64 nb = tid < kGR && rr < a.n ? a.cpre[rr] : 0ull;
  // requests of at most 128 pieces each (max = 10 of short records): all four copied with one round
  // of loads (two pieces per lane and request), loaded now, stored once placed (named registers:
  // a local array here went to scratch)
  bool small = true;
#pragma unroll
  for (u32 q = 0; q < kGQ; ++q) small = small && (bcast_u64(q_nb, q) >> 4) <= 128u;
#define RMQ_GQ_LOAD(q, x0, x1)                                                                        \
  uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;                                                        \
  if (small) {                                                                                        \
    const u64 nbr = bcast_u64(q_nb, q);                                                               \
    const u64 pos0 = bcast_u64(q_pos, q), rw = bcast_u64(q_ring, q);                                  \
    const uint8_t* ring = st.logs + (rw >> 6);                                                        \
    const u64 mask = (1ull << (rw & 63ull)) - 1ull;                                                   \
    if (lane < (nbr >> 4)) x0 = *reinterpret_cast<const uint4*>(ring + ((pos0 + 16ull * lane) & mask)); \
    if (lane + 64u < (nbr >> 4)) x1 = *reinterpret_cast<const uint4*>(ring + ((pos0 + 16ull * (lane + 64u)) & mask)); \
  }
  static_assert(kGQ == 4, "four requests per gather wave");
  RMQ_GQ_LOAD(0, a0, a1)
  RMQ_GQ_LOAD(1, b0, b1)
  RMQ_GQ_LOAD(2, c0_, c1_)
  RMQ_GQ_LOAD(3, d0, d1)
#undef RMQ_GQ_LOAD
  v = bcast_u64(wave_incl_scan(v), 63);  // the wave's sum
  if (lane == 0) s_red[w] = v;
  // this workgroup's requests: exclusive scan of their bytes
  const u64 inc = wave_incl_scan(nb);  // kGR <= 64: one wave holds them all
  __syncthreads();
  const u64 base = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  u64 f0 = 0, f1 = 0, f2 = 0, f3 = 0;  // the final row of request rr (tid < kGR)
  if (tid < kGR && rr < a.n) {
    const u64 pos = base + inc - nb;
    s_pos[tid] = pos;
    u64 w0 = a.res[4 * rr], w2 = a.res[4 * rr + 2], w3 = a.res[4 * rr + 3];  // the resolve's words
    const bool nospc = nb && pos + nb > a.out_cap;
    const int s0 = (int)(uint32_t)w3;
    if (nospc) {  // does not fit: not served (rare); its bytes still count
      w2 = 0;
      w3 = (u64)(uint32_t)kNoSpc;
    }
    f0 = w0;
    f1 = pos;
    f2 = w2;
    f3 = w3;
    if (rr + 1 == a.n)  // bytes needed
      __hip_atomic_store(a.need_host, pos + nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // RMQ_FETCH_COMMIT: the consumer's next offset once its records are in the output (or the
    // first retained offset after RMQ_EOFFSET); every request's offset was read by the resolve
    // kernel before (the host refuses two committing requests for one consumer in a call)
    if (a.commits && (a.req_dev[4 * rr + 3] & 1u)) {
      if (!nospc && (s0 == kOk || s0 == kOffset)) {
        const u32 p = a.req_dev[4 * rr], c = a.req_dev[4 * rr + 1];
        const u64 nx = w0 + (s0 == kOk ? (u64)(uint32_t)w2 : 0ull);
        if (a.replica && (a.req_dev[4 * rr + 3] & kFetchReplica)) {
          a.st.rcur[p] = nx;  // the replica cursor (local: no round carries it)
        } else {
          a.st.cons[(u64)p * a.st.C + c] = nx;
          a.st.cdirty[p] = 1u;  // (with a transport the row travels with the next round)
        }
      }
    }
  }
  if (w == 0) {
    // the final rows into the caller's page-locked rows (or the slot's staging rows): lane j
    // stores half j & 1 of row r0 + j / 2, so one store covers the workgroup's rows contiguously
    // (host rows: whole PCIe writes, not 16-byte pieces at a 32-byte stride)
    static_assert(2 * kGR <= 64, "one wave holds the workgroup's rows");
    const int src = (int)(lane >> 1);
    const u64 x0 = shfl_u64(f0, src), x1 = shfl_u64(f1, src), x2 = shfl_u64(f2, src), x3 = shfl_u64(f3, src);
    if (lane < 2 * kGR && r0 + (lane >> 1) < a.n)
      *reinterpret_cast<ulonglong2*>(a.res_host + 4ull * r0 + 2ull * lane) =
          (lane & 1u) ? make_ulonglong2(x2, x3) : make_ulonglong2(x0, x1);
  }
  __syncthreads();
  // the wave's requests one after the other (one stream of 16-byte pieces per wave: four requests
  // side by side, a quarter-wave or an interleaved run each, measured 1.7x slower at max = 1024)
  const u64 q_out = lane < kGQ ? s_pos[(w * kGQ + lane) & (kGR - 1u)] : 0ull;
  if (small) {
#define RMQ_GQ_STORE(q, x0, x1)                                                                       \
  {                                                                                                   \
    const u64 nbr = bcast_u64(q_nb, q), po = bcast_u64(q_out, q);                                     \
    const bool sv = nbr && po + nbr <= a.out_cap;  /* served (loaded speculatively either way) */   \
    if (sv && lane < (nbr >> 4)) *reinterpret_cast<uint4*>(a.out + po + 16ull * lane) = x0;         \
    if (sv && lane + 64u < (nbr >> 4)) *reinterpret_cast<uint4*>(a.out + po + 16ull * (lane + 64u)) = x1; \
  }
    RMQ_GQ_STORE(0, a0, a1)
    RMQ_GQ_STORE(1, b0, b1)
    RMQ_GQ_STORE(2, c0_, c1_)
    RMQ_GQ_STORE(3, d0, d1)
#undef RMQ_GQ_STORE
    return;
  }
  for (u32 q = 0; q < kGQ; ++q) {
    const u64 nbr = bcast_u64(q_nb, q), pos0_out = bcast_u64(q_out, q);
    if (!nbr || pos0_out + nbr > a.out_cap) continue;  // nothing, past the end, or not served
    const u64 pos0 = bcast_u64(q_pos, q), rw = bcast_u64(q_ring, q);
    const uint8_t* ring = st.logs + (rw >> 6);
    const u64 mask = (1ull << (rw & 63ull)) - 1ull;
    uint8_t* out = a.out + pos0_out;
    const u64 pieces = nbr >> 4;
    u64 p = lane;
    for (; p + 192 < pieces; p += 256) {  // four 16-byte pieces in flight per lane
      const uint4 x0 = *reinterpret_cast<const uint4*>(ring + ((pos0 + 16ull * p) & mask));
      const uint4 x1 = *reinterpret_cast<const uint4*>(ring + ((pos0 + 16ull * (p + 64)) & mask));
      const uint4 x2 = *reinterpret_cast<const uint4*>(ring + ((pos0 + 16ull * (p + 128)) & mask));
      const uint4 x3 = *reinterpret_cast<const uint4*>(ring + ((pos0 + 16ull * (p + 192)) & mask));
      *reinterpret_cast<uint4*>(out + 16ull * p) = x0;
      *reinterpret_cast<uint4*>(out + 16ull * (p + 64)) = x1;
      *reinterpret_cast<uint4*>(out + 16ull * (p + 128)) = x2;
      *reinterpret_cast<uint4*>(out + 16ull * (p + 192)) = x3;
    }
    for (; p < pieces; p += 64)
      *reinterpret_cast<uint4*>(out + 16ull * p) = *reinterpret_cast<const uint4*>(ring + ((pos0 + 16ull * p) & mask));
  }
}

// ---------------------------------------------------------------------------------------------
// Byte budgets (rmq_fetch_bytes, FORMAT.md §7): the kernel between the resolve and the gather of a
// ticket that passes budgets
// ---------------------------------------------------------------------------------------------
constexpr u32 kTT = 256;       // threads per trim workgroup
constexpr u32 kTQ = 64 / kQL;  // requests per trim wave: a quarter-wave each

// load_window's pieces, but only those at or before `limit` (the others read as empty records: the
// walk never consults them).
__device__ __forceinline__ WinWords load_window_to(const uint8_t* ring, u64 wb, u32 hl, u64 mask, u64 limit) {
  WinWords x{};
#pragma unroll
  for (u32 k = 0; k < kPPL; ++k) {
    const u64 p = wb + 16ull * (kPPL * hl + k);
    if (p <= limit) x.w[k] = *reinterpret_cast<const u32*>(ring + ((p + 8ull) & mask));
  }
  return x;
}

// A quarter-wave per request (16,384 requests: 4,096 waves, one round of the resident waves). A
// request served RMQ_OK with records whose bytes exceed its budget b is cut at X, the largest
// record start in [pos0, limit], limit = pos0 + (b & ~15): records and positions are 16-byte
// aligned, so the records before X are exactly the k* whose bytes are at most b. The sparse index
// is keyed by position (E[m] = first record start at or after m I, rising with m): the largest m of
// [ceil(pos0 / I), floor(limit / I)] with E[m].pos <= limit is searched from the top, 16 probes a
// round (the first round the 16 highest entries: it ends the search unless a record spans 16
// intervals or more; then 16-ary over what is left below), and from that entry (or from the slice
// start) the length words up to the limit are read as header windows and walked in registers.
// Trust, as the resolve's: an entry starts the walk only if it is 16-byte aligned, lies in
// [pos0, limit] and its offset inside the slice (and it names the slice's first record iff it
// names its position); the walk reads length words at positions in [pos0, limit] only, every
// address masked into the ring, stops at the first record that ends past the limit and never
// counts the slice's last record, so a damaged length word cuts early and is never followed out
// of the slice.
// The cut itself, shared by the trim and the fill kernel: the whole wave calls it, quarter q cuts
// request r (quarter-uniform) at budget b when act (the caller has checked: served RMQ_OK with
// count > 0 records, bytes > b), rewrites the row's words, cpre and the position cache entry, and
// returns the k* records and bytes kept. zst: the status of a row of which not even the first
// record fits (its size goes into `reserved`).
struct TrimCut {
  u64 k, nb;
};
__device__ __forceinline__ TrimCut trim_request(const FetchTrimArgs& a, u32 r, bool act, u64 b, u64 count, u64 bytes,
                                                int zst) {
  const DevState& st = a.st;
  const u32 lane = lane_id(), q = lane / kQL, hl = lane % kQL;
  const u64 off = act ? a.res[4ull * r] : 0ull;
  const u64 pos0 = act ? a.aux[2ull * r] : 0ull, rw = act ? a.aux[2ull * r + 1] : 0ull;
  const u32 p = act ? a.req_dev[4ull * r] : 0u, c = act ? a.req_dev[4ull * r + 1] : 0u;  // (served: in range)
  const u32 ilog = st.interval_log2;
  const RingRef rg = ring_ref(act ? st.ring[p] : 0ull, ilog, st.icap_mul);
  const uint8_t* ring = st.logs + (rw >> 6);
  const u64 mask = (1ull << (rw & 63ull)) - 1ull;
  const u64* E = st.index + rg.ibase * 2;
  const u64 limit = pos0 + (b & ~15ull);
  constexpr u32 kQMask = (1u << kQL) - 1u;
  // the index entry to start from (quarter-uniform state)
  u64 c_off = off, c_pos = pos0;
  long lo = (long)((pos0 + (1ull << ilog) - 1ull) >> ilog), hi = (long)(limit >> ilog), step = 1;
  bool open = act && lo <= hi;
  while (__any(open)) {
    const long m = hi - (long)hl * step;  // probes from the top of the range
    bool ok = false;
    u64 eo = 0, ep = 0;
    if (open && m >= lo) {
      const u64* e = E + ((u64)m % rg.icap) * 2;
      eo = e[0];
      ep = e[1];
      ok = !(ep & 15ull) && ep >= pos0 && ep <= limit && eo >= off && eo < off + count && ((eo == off) == (ep == pos0));
    }
    const u32 bal = (u32)(__ballot(ok) >> (kQL * q)) & kQMask;  // this quarter's probes
    const u32 top = bal ? (u32)__builtin_ctz(bal) : 0u;          // the highest entry at or before the limit
    const u64 so = shfl_u64(eo, (int)(kQL * q + top)), sp = shfl_u64(ep, (int)(kQL * q + top));
    if (open) {
      if (!bal) {  // every probe past the limit: the answer lies below this round's lowest probe
        hi -= (long)(kQL - 1) * step + 1;
      } else {
        c_off = so;
        c_pos = sp;
        const long mk = hi - (long)top * step;
        lo = mk + 1;  // that probe, or an entry between it and the probe above it
        hi = step == 1 ? mk : min(hi, mk + step - 1);
      }
      open = lo <= hi;
      step = (hi - lo + (long)kQL) / (long)kQL;
    }
  }
  // the walk: records from c_pos while they end at or before the limit
  constexpr u32 kWin = kPPL * kQL;  // pieces per header window
  u64 wb = c_pos, cur = 0, k = c_off - off, rs_last = 0;
  WinWords Lw{};
  if (act) Lw = load_window_to(ring, wb, hl, mask, limit);
  bool go = act;
  while (__any(go)) {
    const bool mv = go && cur >= kWin;  // quarter-uniform: the quarter walked off its window
    if (__any(mv)) {
      if (mv) {
        wb += 16ull * cur;
        cur = 0;
        Lw = load_window_to(ring, wb, hl, mask, limit);
      }
    }
    const u32 src = kQL * q + ((u32)cur / kPPL);
    u32 len = 0;
#pragma unroll
    for (u32 j = 0; j < kPPL; ++j) {
      const u32 x = (u32)__shfl((int)Lw.w[j], (int)(src & 63u), 64);
      len = ((u32)cur % kPPL) == j ? x : len;
    }
    if (go) {
      const u64 rs = 16ull + (((u64)len + 15ull) & ~15ull);
      if (wb + 16ull * cur + rs <= limit && k + 1 < count) {
        cur += rs >> 4;
        ++k;
      } else {
        go = false;
        rs_last = rs;
      }
    }
  }
  const u64 nb = k ? wb + 16ull * cur - pos0 : 0ull;  // the trimmed slice's bytes
  if (act && hl == 0) {
    a.res[4ull * r + 2] = k | (nb << 32);
    // no record fits: not served (zst) for this request alone, the first record's size in `reserved`
    if (!k) a.res[4ull * r + 3] = (u64)(uint32_t)zst | ((rs_last < bytes ? rs_last : bytes) << 32);
    a.cpre[r] = (u32)nb;
    *reinterpret_cast<ulonglong2*>(st.pcache + ((u64)p * st.C + c) * 2) = make_ulonglong2(off + k, pos0 + nb);
  }
  return TrimCut{k, nb};
}

// The trim kernel: every budgeted request that is served more than its budget is cut.
__global__ __launch_bounds__(kTT) void fetch_trim_kernel(FetchTrimArgs a) {
  const u32 lane = lane_id(), q = lane / kQL;
  const u32 r0 = (blockIdx.x * (kTT / 64) + (threadIdx.x >> 6)) * kTQ;  // the wave's first request
  const u32 r = r0 + q;
  const bool live = r < a.n;
  // one read of the request's words (the same address in the 16 lanes of a quarter)
  const u32 b = live ? a.budget[r] : 0u;
  const u64 w2 = live ? a.res[4ull * r + 2] : 0ull, w3 = live ? a.res[4ull * r + 3] : 0ull;
  const u64 count = (u32)w2, bytes = w2 >> 32;
  const bool act = live && b != 0u && (int)(u32)w3 == kOk && count > 0 && bytes > (u64)b;
  if (!__any(act)) return;
  const TrimCut t = trim_request(a, r, act, b, count, bytes, kNoSpc);
  // the bytes removed leave the chunk's sum: one subtract per wave (its requests share a chunk)
  static_assert(kFetchChunk % kTQ == 0, "a trim wave never straddles a chunk");
  u64 cut = act ? bytes - t.nb : 0ull, cut_w = 0;
#pragma unroll
  for (u32 j = 0; j < kTQ; ++j) cut_w += bcast_u64(cut, kQL * j);
  if (lane == 0 && cut_w)
    atomicAdd((unsigned long long*)&a.csum[(u64)(r0 / kFetchChunk) * kCsumStride], (unsigned long long)(0ull - cut_w));
}

// ---------------------------------------------------------------------------------------------
// RMQ_FETCH_FILL (FORMAT.md §7 "Filling a bounded output"): the kernel before the gather of a ticket
// that fills its output
// ---------------------------------------------------------------------------------------------
constexpr int kPending = 1;  // RMQ_PENDING

// A workgroup per chunk of kFetchChunk requests, a thread per request; every chunk decides alone.
// With B_r = cpre[r] (not zero for exactly the rows served RMQ_OK with records, the trim's cuts
// applied) and P_r the bytes of the requests before r (the chunk sums before the chunk, then a scan
// of the chunk's cpre), the request that crosses the end of the output is the one with B_r > 0,
// P_r <= out_cap < P_r + B_r (the sums rise with r, so there is at most one and every row knows
// by itself which side of it it stands on): it is cut at budget out_cap - P_r by the trim's own
// search and walk (quarter 0 of wave 0), and every served row after it (P_r > out_cap) becomes
// RMQ_PENDING with the true pair {its offset, that offset's position} back in the position cache.
// A chunk wholly inside the output changes nothing, one wholly past it holds pending rows only.
// The chunk sums are read in t.csum and written, every chunk's, to csum_out, which no workgroup
// of this kernel reads: a chunk's new sum never meets another workgroup's read of its old one.
__global__ __launch_bounds__(kFetchChunk) void fetch_fill_kernel(FetchFillArgs a) {
  static_assert(kFetchChunk == 256, "four waves, a thread per request of the chunk");
  const FetchTrimArgs& t = a.t;
  const u32 c = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  __shared__ u64 s_sum[kFetchChunk / 64];
  __shared__ u64 s_cutp;  // P of the crossing request
  __shared__ u32 s_cutr;  // its index (~0: none)
  // bytes before the chunk (every wave on its own: at most a few loads per lane, L2-resident)
  u64 base = 0;
  for (u32 k = lane; k < c; k += 64) base += t.csum[(u64)k * kCsumStride];
  base = bcast_u64(wave_incl_scan(base), 63);
  const u64 own = t.csum[(u64)c * kCsumStride];
  if (base + own <= a.out_cap) {  // (workgroup-uniform) wholly inside: as resolved
    if (tid == 0) a.csum_out[(u64)c * kCsumStride] = own;
    return;
  }
  const u32 r = c * kFetchChunk + tid;
  const u64 nb = r < t.n ? t.cpre[r] : 0ull;
  const u64 inc = wave_incl_scan(nb);
  if (lane == 63) s_sum[w] = inc;
  if (tid == 0) s_cutr = ~0u;
  __syncthreads();
  u64 P = base + inc - nb;
  for (u32 k = 0; k < w; ++k) P += s_sum[k];
  const bool pend = nb && P > a.out_cap;
  if (nb && P <= a.out_cap && P + nb > a.out_cap) {
    s_cutr = r;
    s_cutp = P;
  }
  if (pend) {
    const u32 p = t.req_dev[4ull * r], cn = t.req_dev[4ull * r + 1];  // (served: in range)
    const bool vf = a.verify && (t.req_dev[4ull * r + 3] & kFetchVerify);
    const u64 off = t.res[4ull * r], pos0 = t.aux[2ull * r];
    t.res[4ull * r + 2] = 0;
    t.res[4ull * r + 3] = (u64)(uint32_t)kPending;
    t.cpre[r] = 0;
    // (a flagged request that is not served leaves no entry, as the verify kernel has it: FORMAT.md §10)
    *reinterpret_cast<ulonglong2*>(t.st.pcache + ((u64)p * t.st.C + cn) * 2) =
        vf ? make_ulonglong2(~0ull, 0ull) : make_ulonglong2(off, pos0);
  }
  __syncthreads();
  if (w != 0) return;
  const u32 rc = s_cutr;
  const bool act = rc != ~0u && lane < kQL;
  u64 kept = base > a.out_cap ? 0ull : own;  // (no crossing request: only if the sums disagree with cpre)
  if (rc != ~0u) {
    const u64 Pc = s_cutp;
    const u64 w2 = t.res[4ull * rc + 2];
    // an output that cannot hold the call's first record: RMQ_ENOSPC, the capacity that would in `reserved`
    const TrimCut x = trim_request(t, rc, act, a.out_cap - Pc, (u32)w2, w2 >> 32, Pc ? kPending : kNoSpc);
    if (lane == 0 && !x.k && a.verify && (t.req_dev[4ull * rc + 3] & kFetchVerify))
      *reinterpret_cast<ulonglong2*>(t.st.pcache + ((u64)t.req_dev[4ull * rc] * t.st.C + t.req_dev[4ull * rc + 1]) * 2) =
          make_ulonglong2(~0ull, 0ull);
    kept = Pc - base + bcast_u64(x.nb, 0);
  }
  if (lane == 0) a.csum_out[(u64)c * kCsumStride] = kept;
}

// ---------------------------------------------------------------------------------------------
// RMQ_FETCH_VERIFY (FORMAT.md §10): the third kernel of a ticket with a flagged request
// ---------------------------------------------------------------------------------------------
constexpr int kCorrupt = -10;
constexpr u32 kVT = 256;        // threads per verify workgroup: a wave per request
constexpr u32 kBigVerify = 64;  // records over this many 16-byte pieces: the whole wave (as the scrub)

// The length words of pieces 64 k .. 64 k + 63 of a slice of nb16 pieces (lane l: piece 64 k + l).
__device__ __forceinline__ u32 slice_lens(const uint8_t* base, u64 nb16, u64 k, u32 lane) {
  const u64 piece = 64ull * k + lane;
  return piece < nb16 ? *reinterpret_cast<const u32*>(base + 16ull * piece + 8ull) : 0u;
}

// Whether the nb16 pieces at base are `count` FORMAT.md §1 records with header offsets start,
// start + 1, ..., back to back and filling the slice exactly, each with its CRC32C and zero padding
// (wave-uniform arguments and result). The record starts come from walking the length words, read
// cooperatively as windows of 64 pieces (the next window in flight while one is walked); then a
// lane per record, 64 at a time. Nothing outside the slice is read: a window piece, a header and
// every payload piece are loaded only at piece indices below nb16, and a record's piece count is
// clamped by the pieces left after its header before any of them is loaded.
__device__ __forceinline__ bool verify_slice(const CrcConsts* crc, const u32 (*t8)[256], const uint8_t* base,
                                             u64 nb16, u64 start, u64 count) {
  const u32 lane = lane_id();
  u64 q = 0, done = 0;  // piece of the next record start; records checked (both wave-uniform)
  u64 wk = 0;
  u32 W0 = slice_lens(base, nb16, 0, lane), W1 = slice_lens(base, nb16, 1, lane);
  bool bad = false;
  while (q < nb16 && !bad) {
    // the next (at most 64) record starts: lane j keeps the start of record done + j
    u64 myq = 0;
    u32 nrec = 0;
    while (nrec < 64u && q < nb16) {
      const u64 k = q >> 6;
      if (k != wk) {
        W0 = k == wk + 1ull ? W1 : slice_lens(base, nb16, k, lane);
        W1 = slice_lens(base, nb16, k + 1ull, lane);
        wk = k;
      }
      const u32 Lq = (u32)__shfl((int)W0, (int)(q & 63ull), 64);
      if (lane == nrec) myq = q;
      q += 1ull + (Lq >> 4) + ((Lq & 15u) ? 1u : 0u);
      ++nrec;
    }
    q = bcast_u64(q, 0);  // (uniform by construction)
    const bool in = lane < nrec;
    uint4 hdr = make_uint4(0, 0, 0, 0);
    u32 L = 0, m = 0;
    bool chk = false;
    if (in) {
      hdr = *reinterpret_cast<const uint4*>(base + 16ull * myq);
      L = hdr.z;
      m = (L >> 4) + ((L & 15u) ? 1u : 0u);
      const u64 off = ((u64)hdr.y << 32) | hdr.x;
      chk = off == start + done + lane && done + lane < count && (u64)m <= nb16 - myq - 1ull;
    }
    bool fail = in && !chk;
    const bool big = chk && m > kBigVerify;
    const u32 mm = chk && !big ? m : 0u;
    const uint8_t* pay = base + 16ull * (myq + 1ull);
    u32 acc = 0xFFFFFFFFu;
    bool padz = true;
    for (u32 c = 0; __any(c < mm); c += 4) {
      uint4 v[4];
#pragma unroll
      for (u32 u = 0; u < 4; ++u)  // four pieces in flight per lane
        v[u] = c + u < mm ? *reinterpret_cast<const uint4*>(pay + 16ull * (c + u)) : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (u32 u = 0; u < 4; ++u)
        if (c + u < mm) {
          acc = crc_step8(t8, crc_step8(t8, acc, v[u].x, v[u].y), v[u].z, v[u].w);
          if (c + u + 1u == mm) padz = pad_zero16(v[u], L);
        }
    }
    for (u64 bm = __ballot(big); bm; bm &= bm - 1ull) {
      const u32 sl = (u32)__builtin_ctzll(bm);
      const uint8_t* bpay = reinterpret_cast<const uint8_t*>(bcast_u64(reinterpret_cast<u64>(pay), sl));
      const u32 bm16 = (u32)__builtin_amdgcn_readlane((int)m, (int)sl);  // (at most the slice's pieces)
      const u32 bacc = wave_crc_pieces(crc, t8, bm16,
                                       [&](u32 jp) { return *reinterpret_cast<const uint4*>(bpay + 16ull * jp); });
      if (lane == sl) acc = bacc;
    }
    if (chk) {
      if (big) padz = pad_zero16(*reinterpret_cast<const uint4*>(pay + 16ull * (m - 1u)), L);
      fail = crc_of_padded(crc, acc, L, m) != hdr.w || !padz;
    }
    bad = __any(fail);
    done += nrec;
  }
  return !bad && q == nb16 && done == count;
}

// A wave per request of the ticket (a grid of at most a few workgroups per CU, the waves striding
// over the requests): a flagged request served RMQ_OK with records is checked in the output and,
// if a record fails, its row rewritten RMQ_ECORRUPT with count 0 (start_offset, out_pos and bytes
// stay); then the commit the gather left to this kernel, with the gather's exact rule.
__global__ __launch_bounds__(kVT, 4) void fetch_verify_kernel(FetchVerifyArgs a) {
  __shared__ __attribute__((aligned(16))) u32 tabs[16 * 256];  // table[8] then zshift[2][4]
  __shared__ __attribute__((aligned(16))) u32 nibs[512];
  crc_tables_lds<kVT>(a.crc, tabs, nibs);
  __syncthreads();
  const u32(*t8)[256] = reinterpret_cast<const u32(*)[256]>(tabs);
  const u32 lane = lane_id();
  const u32 stride = gridDim.x * (kVT / 64);
  for (u32 r = (u32)__builtin_amdgcn_readfirstlane(blockIdx.x * (kVT / 64) + (threadIdx.x >> 6)); r < a.n; r += stride) {
    const u32 flags = a.req_dev[4ull * r + 3];
    if (!(flags & (kFetchVerify | 1u))) continue;  // neither checked nor committed
    const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(a.rows + 4ull * r);
    const ulonglong2 hi = *reinterpret_cast<const ulonglong2*>(a.rows + 4ull * r + 2);
    const u64 w0 = bcast_u64(lo.x, 0), w1 = bcast_u64(lo.y, 0), w2 = bcast_u64(hi.x, 0);
    const int status = (int)(u32)bcast_u64(hi.y, 0);
    const u64 count = (u32)w2, bytes = w2 >> 32;
    bool refused = false;
    if ((flags & kFetchVerify) && status == kOk && count) {
      refused = !verify_slice(a.crc, t8, a.out + w1, bytes >> 4, w0, count);
      if (refused && lane == 0)
        *reinterpret_cast<ulonglong2*>(a.rows + 4ull * r + 2) = make_ulonglong2(bytes << 32, (u64)(uint32_t)kCorrupt);
    }
    // A flagged request that is not served, refused here or too large for the output (its size
    // comes from the same walk), leaves no position cache entry: the resolve stored one from length
    // words nothing has checked, so the consumer's next fetch takes the index search (FORMAT.md
    // §10; the resolve found records for both, so their partition and consumer are in range)
    if ((flags & kFetchVerify) && (refused || status == kNoSpc) && lane == 0) {
      const u32 p = a.req_dev[4ull * r], c = a.req_dev[4ull * r + 1];
      if (p < a.st.P && c < a.st.C)
        *reinterpret_cast<ulonglong2*>(a.st.pcache + ((u64)p * a.st.C + c) * 2) = make_ulonglong2(~0ull, 0ull);
    }
    // RMQ_FETCH_COMMIT, as the gather does it (a request that did not fit has status RMQ_ENOSPC here)
    if (a.commits && (flags & 1u) && !refused && (status == kOk || status == kOffset) && lane == 0) {
      const u32 p = a.req_dev[4ull * r], c = a.req_dev[4ull * r + 1];
      const u64 nx = w0 + (status == kOk ? count : 0ull);
      if (a.replica && (flags & kFetchReplica)) {
        a.st.rcur[p] = nx;
      } else {
        a.st.cons[(u64)p * a.st.C + c] = nx;
        a.st.cdirty[p] = 1u;
      }
    }
  }
}

void launch_fetch_verify(const FetchVerifyArgs& a, uint32_t max_wgs, hipStream_t s) {
  if (!a.n) return;
  const uint32_t wgs = std::min<uint32_t>((a.n + kVT / 64 - 1) / (kVT / 64), std::max<uint32_t>(max_wgs, 1u));
  hipLaunchKernelGGL(fetch_verify_kernel, dim3(wgs), dim3(kVT), 0, s, a);
}

// ---------------------------------------------------------------------------------------------
// Record table (rmq_fetch_table, FORMAT.md §7 "Record table"): the kernels after the gather (and
// the verify) of a ticket that asks for one
// ---------------------------------------------------------------------------------------------
constexpr u32 kTW = 256;  // threads per table-walk workgroup: a wave per request

// The words row r owns, from its final words {count | bytes << 32, status}: count + 1 if it is
// served RMQ_OK with records, else none.
__device__ __forceinline__ u64 table_words(u64 w2, u64 w3) { return (int)(u32)w3 == kOk && (u32)w2 ? (u64)(u32)w2 + 1ull : 0ull; }

// Scan, first half: a workgroup per chunk of kFetchChunk rows, a thread per row: each row's words
// into rec_row[r] (the second half turns them into their prefix in place), the chunk's into tsum.
__global__ __launch_bounds__(kFetchChunk) void fetch_table_sum_kernel(FetchTableArgs a) {
  const u32 c = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  __shared__ u64 s_sum[kFetchChunk / 64];
  const u32 r = c * kFetchChunk + tid;
  u64 tw = 0;
  if (r < a.n) {
    const ulonglong2 hi = *reinterpret_cast<const ulonglong2*>(a.rows + 4ull * r + 2);
    tw = table_words(hi.x, hi.y);
    a.rec_row[r] = tw;
  }
  const u64 inc = wave_incl_scan(tw);
  if (lane == 63) s_sum[w] = inc;
  __syncthreads();
  if (tid == 0) a.tsum[c] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// Scan, second half: the same grid; the words before the chunk from the chunk sums (every wave on
// its own, as the fill kernel reads its sums), an exclusive scan of the chunk's rows, rec_row[r]
// rewritten in place by the thread that read it; the last row's thread adds rec_row[n] and tells the
// host. Sums of integers in a fixed order: the same table from the same rows, run after run.
__global__ __launch_bounds__(kFetchChunk) void fetch_table_rows_kernel(FetchTableArgs a) {
  static_assert(kFetchChunk == 256, "four waves, a thread per row of the chunk");
  const u32 c = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  __shared__ u64 s_sum[kFetchChunk / 64];
  u64 base = 0;
  for (u32 k = lane; k < c; k += 64) base += a.tsum[k];
  base = bcast_u64(wave_incl_scan(base), 63);
  const u32 r = c * kFetchChunk + tid;
  const u64 tw = r < a.n ? a.rec_row[r] : 0ull;
  const u64 inc = wave_incl_scan(tw);
  if (lane == 63) s_sum[w] = inc;
  __syncthreads();
  u64 P = base + inc - tw;
  for (u32 k = 0; k < w; ++k) P += s_sum[k];
  if (r < a.n) a.rec_row[r] = P;
  if (r + 1 == a.n) {
    a.rec_row[a.n] = P + tw;
    __hip_atomic_store(a.need_host, P + tw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// The table of one run (wave-uniform arguments): the nb16 pieces at base hold `count` records;
// words[k], k < count, gets the byte position of record k and words[count] the run's bytes. The
// walk is verify_slice's: the length words read as windows of 64 pieces, the next window in flight
// while one is walked, lane j keeping the start of record done + j, then one 8-byte store per lane
// for the round's (at most 64) records. Nothing here trusts a length word: slice_lens loads no piece
// at or beyond nb16, table_next never steps past nb16, and a walk that reaches nb16 before `count`
// records (a damaged length word) ends there with the words left set to the run's bytes. Exactly
// the words [0, count] are written.
__device__ __forceinline__ void table_walk(const uint8_t* base, u32 nb16, u32 count, u64* words) {
  const u32 lane = lane_id();
  // piece of the next record start; records placed; window (all wave-uniform, and 32-bit: a row's
  // bytes are a 32-bit word, so nb16 < 2^28 and table_next<u32> cannot wrap)
  u32 q = 0, done = 0, wk = 0;
  u32 W0 = slice_lens(base, nb16, 0, lane), W1 = slice_lens(base, nb16, 1, lane);
  while (done < count && q < nb16) {
    u32 myq = 0, nrec = 0;
    const u32 lim = count - done < 64u ? count - done : 64u;
    while (nrec < lim && q < nb16) {
      const u32 k = q >> 6;
      if (k != wk) {
        W0 = k == wk + 1u ? W1 : slice_lens(base, nb16, k, lane);
        W1 = slice_lens(base, nb16, (u64)k + 1ull, lane);
        wk = k;
      }
      const u32 Lq = (u32)__builtin_amdgcn_readlane((int)W0, __builtin_amdgcn_readfirstlane((int)(q & 63u)));
      myq = lane == nrec ? q : myq;
      q = table_next<u32>(q, Lq, nb16);
      ++nrec;
    }
    if (lane < nrec) words[(u64)done + lane] = 16ull * myq;
    done += nrec;
  }
  for (u64 k = (u64)done + lane; k <= count; k += 64) words[k] = 16ull * nb16;  // the end word (and an early end's rest)
}

// A wave per request, the waves striding over the requests on a bounded grid (the verify kernel's
// shape): a row that owns words, all of them inside rec_cap, has its run walked.
__global__ __launch_bounds__(kTW) void fetch_table_walk_kernel(FetchTableArgs a) {
  const u32 stride = gridDim.x * (kTW / 64);
  for (u32 r = (u32)__builtin_amdgcn_readfirstlane(blockIdx.x * (kTW / 64) + (threadIdx.x >> 6)); r < a.n; r += stride) {
    const ulonglong2 lo = *reinterpret_cast<const ulonglong2*>(a.rows + 4ull * r);
    const ulonglong2 hi = *reinterpret_cast<const ulonglong2*>(a.rows + 4ull * r + 2);
    const u64 w1 = bcast_u64(lo.y, 0), w2 = bcast_u64(hi.x, 0), w3 = bcast_u64(hi.y, 0);
    const u64 tw = table_words(w2, w3);
    if (!tw) continue;
    const u64 t0 = bcast_u64(a.rec_row[r], 0);
    if (t0 > a.rec_cap || tw > a.rec_cap - t0) continue;  // its words do not fit: none of them written
    table_walk(a.out + w1, (u32)(w2 >> 36), (u32)w2, a.rec_pos + t0);
  }
}

void launch_fetch_table(const FetchTableArgs& a, uint32_t max_wgs, hipStream_t s) {
  if (!a.n) return;
  const dim3 chunks((a.n + kFetchChunk - 1) / kFetchChunk);
  hipLaunchKernelGGL(fetch_table_sum_kernel, chunks, dim3(kFetchChunk), 0, s, a);
  hipLaunchKernelGGL(fetch_table_rows_kernel, chunks, dim3(kFetchChunk), 0, s, a);
  if (!a.rec_cap) return;  // a size probe
  const uint32_t wgs = std::min<uint32_t>((a.n + kTW / 64 - 1) / (kTW / 64), std::max<uint32_t>(max_wgs, 1u));
  hipLaunchKernelGGL(fetch_table_walk_kernel, dim3(wgs), dim3(kTW), 0, s, a);
}

// ---------------------------------------------------------------------------------------------
// rmq_lag (FORMAT.md §7 "Lag"): how far behind a reader is, in records and bytes, and how many bytes
// its partition can still take before retention evicts what it has not read
// ---------------------------------------------------------------------------------------------
static_assert(kLagRows == kRW * kRPW, "the lag kernel has the resolve's shape");

// The resolve's shape: a half-wave per row, two per wave; the workgroup's rows (and their explicit
// offsets) read once by consecutive 16-byte (8-byte) loads through LDS; every word of the partition
// in one round; the positions of the slice's two ends, record start_offset and record
// high_watermark, found together by a quarter-wave each with the resolve's own search
// (record_posq, no position cache: nothing here is keyed by a consumer's last slice). The row
// arithmetic is lag_row.hpp's, all of it 64-bit. Each row leaves as one 64-byte record, four
// 16-byte stores of consecutive lanes. Nothing of the engine is written.
__global__ __launch_bounds__(64 * kRW) void lag_kernel(LagArgs a) {
  const DevState& st = a.st;
  const u32 lane = lane_id(), w = threadIdx.x >> 6;
  const u32 r = (blockIdx.x * kRW + w) * kRPW + (lane >> 5);
  const bool live = r < a.n;  // (no early return: the workgroup meets at the barrier below)
  __shared__ uint4 s_rq[kLagRows];
  __shared__ u64 s_at[kLagRows];
  {
    const u32 r0 = blockIdx.x * kLagRows + threadIdx.x;
    if (threadIdx.x < kLagRows && r0 < a.n) {
      const uint4 x = *reinterpret_cast<const uint4*>(a.req + 4ull * r0);
      s_at[threadIdx.x] = a.at ? a.at[r0] : ~0ull;
      s_rq[threadIdx.x] = x;
    }
  }
  __syncthreads();
  const uint4 rq = live ? s_rq[w * kRPW + (lane >> 5)] : make_uint4(0, 0, 0, 0);
  const u64 at = live ? s_at[w * kRPW + (lane >> 5)] : ~0ull;
  const u32 p = rq.x, c = rq.y;
  const bool okp = live && p < st.P;
  const u32 pp = okp ? p : 0u, cc = c < st.C ? c : 0u;
  const u32 lead = okp ? st.is_leader[pp] : 0u;
  const bool rep = (rq.w & kFetchReplica) != 0;  // (max_records and every other flag bit: not read)
  const u64 tab = okp ? (rep ? st.rcur[pp] : st.cons[(u64)pp * st.C + cc]) : 0ull;
  const u64 hw = okp ? st.hw[pp] : 0ull;
  PartView v;
  v.leo = okp ? st.leo[pp] : 0ull;
  v.used = okp ? st.used[pp] : 0ull;
  v.start_off = okp ? st.start_off[pp] : 0ull;
  v.start_pos = okp ? st.start_pos[pp] : 0ull;
  const u32 lm = okp ? st.local_mask[pp] : 0u;
  const u64 desc = okp ? st.ring[pp] : 0ull;
  const u64 off = okp && at != ~0ull ? at : tab;
  v.rg = ring_ref(desc, st.interval_log2, st.icap_mul);
  v.ring = st.logs;
  int status = kOk;
  LagPlan pl{0, 0, 0, kOk};
  bool ok = false;  // the row passed the checks
  if (!live) {
  } else if (p >= st.P) {
    status = kNoPart;
  } else if (!lead && !rep) {
    status = kNotLeader;
  } else if (c >= st.C) {
    status = kInval;
  } else {
    pl = lag_plan(off, hw, v.start_off);
    ok = true;
  }
  const bool need = ok && pl.records > 0;  // both ends are searched
  if (need) {
    const u32 r0 = lm ? (u32)__ffs(lm) - 1u : 0u;
    v.ring = st.logs + (u64)r0 * st.rstride + v.rg.base;
  }
  // quarter 0 of the half: record start_offset, quarter 1: record high_watermark
  const u32 hb = lane & 32u;
  const u64 pq = record_posq(st, v, (lane & 16u) ? hw : pl.start_offset, need, false, 0ull, 0ull);
  const u64 pos0 = __shfl(pq, (int)hb, 64), pend = __shfl(pq, (int)(hb + 16u), 64);
  LagRow row{0, 0, 0, 0, 0, 0, kLagNone, status};
  if (ok) row = lag_row(pl, pos0, pend, v.start_pos, v.used, v.rg.seg, st.interval_log2);
  static_assert(sizeof(LagRow) >= 60, "seven words and the status");
  const u32 j = lane & 31u;
  if (live && j < 4u) {
    const u64 x0 = j == 0u ? row.start_offset : j == 1u ? row.bytes : j == 2u ? row.start_pos : row.headroom;
    const u64 x1 = j == 0u ? row.records : j == 1u ? row.evicted : j == 2u ? row.end_pos : (u64)(uint32_t)row.status;
    *reinterpret_cast<ulonglong2*>(a.res + 8ull * r + 2ull * j) = make_ulonglong2(x0, x1);
  }
}

void launch_lag(const LagArgs& a, hipStream_t s) {
  if (!a.n) return;
  hipLaunchKernelGGL(lag_kernel, dim3((a.n + kLagRows - 1) / kLagRows), dim3(64 * kRW), 0, s, a);
}

// ev[4]: start / end events of the two kernels, recorded by the dispatches themselves
// (profiling: kernel time without the host's launch gaps), or null
// Load the fetch kernels' code at engine creation (a process's first launch of a kernel otherwise
// loads it: ~20 ms inside the first rmq_fetch, profiles/r03q_prof).
void preload_fetch_kernels() {
  hipFuncAttributes fa;
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_resolve_kernel<false>));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_gather_kernel<false>));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_resolve_kernel<true>));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_gather_kernel<true>));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_trim_kernel));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_resolve_kernel<false, true>));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_fill_kernel));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_table_sum_kernel));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_table_rows_kernel));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&fetch_table_walk_kernel));
  (void)hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(&lag_kernel));
}

static void launch_batch(const FetchBatch& b, hipStream_t s, const hipEvent_t* e) {
  if (!b.rwg0[b.nt]) return;
  if (b.nt == 1) {  // one ticket: the 4x smaller kernarg, fixed offsets
    if (b.t[0].at)  // explicit offsets (rmq_fetch_at): the resolve that reads them
      hipExtLaunchKernelGGL((fetch_resolve_kernel<false, true>), dim3(b.rwg0[1]), dim3(64 * kRW), 0, s,
                            e ? e[0] : nullptr, e ? e[1] : nullptr, 0, b.t[0]);
    else
      hipExtLaunchKernelGGL(fetch_resolve_kernel<false>, dim3(b.rwg0[1]), dim3(64 * kRW), 0, s, e ? e[0] : nullptr,
                            e ? e[1] : nullptr, 0, b.t[0]);
    hipExtLaunchKernelGGL(fetch_gather_kernel<false>, dim3(b.gwg0[1]), dim3(64 * kFW), 0, s, e ? e[2] : nullptr,
                          e ? e[3] : nullptr, 0, b.t[0]);
    return;
  }
  hipExtLaunchKernelGGL(fetch_resolve_kernel<true>, dim3(b.rwg0[b.nt]), dim3(64 * kRW), 0, s, e ? e[0] : nullptr,
                        e ? e[1] : nullptr, 0, b);
  hipExtLaunchKernelGGL(fetch_gather_kernel<true>, dim3(b.gwg0[b.nt]), dim3(64 * kFW), 0, s, e ? e[2] : nullptr,
                        e ? e[3] : nullptr, 0, b);
}

void launch_fetch_batch(const FetchArgs* t, uint32_t nt, hipStream_t s) {
  FetchBatch b{};
  b.nt = nt;
  for (uint32_t k = 0; k < nt; ++k) {
    b.t[k] = t[k];
    b.rwg0[k + 1] = b.rwg0[k] + (t[k].n + kRW * kRPW - 1) / (kRW * kRPW);
    b.gwg0[k + 1] = b.gwg0[k] + (t[k].n + kGR - 1) / kGR;
  }
  launch_batch(b, s, nullptr);
}

void launch_fetch_budget(const FetchArgs& a, const FetchTrimArgs& t, hipStream_t s) {
  if (!a.n) return;
  const dim3 rwgs((a.n + kRW * kRPW - 1) / (kRW * kRPW));
  if (a.at)
    hipLaunchKernelGGL((fetch_resolve_kernel<false, true>), rwgs, dim3(64 * kRW), 0, s, a);
  else
    hipLaunchKernelGGL(fetch_resolve_kernel<false>, rwgs, dim3(64 * kRW), 0, s, a);
  hipLaunchKernelGGL(fetch_trim_kernel, dim3((a.n + (kTT / 64) * kTQ - 1) / ((kTT / 64) * kTQ)), dim3(kTT), 0, s, t);
  hipLaunchKernelGGL(fetch_gather_kernel<false>, dim3((a.n + kGR - 1) / kGR), dim3(64 * kFW), 0, s, a);
}

void launch_fetch_fill(const FetchArgs& a, const FetchFillArgs& f, hipStream_t s) {
  if (!a.n) return;
  const dim3 rwgs((a.n + kRW * kRPW - 1) / (kRW * kRPW));
  if (a.at)
    hipLaunchKernelGGL((fetch_resolve_kernel<false, true>), rwgs, dim3(64 * kRW), 0, s, a);
  else
    hipLaunchKernelGGL(fetch_resolve_kernel<false>, rwgs, dim3(64 * kRW), 0, s, a);
  if (f.t.budget)
    hipLaunchKernelGGL(fetch_trim_kernel, dim3((a.n + (kTT / 64) * kTQ - 1) / ((kTT / 64) * kTQ)), dim3(kTT), 0, s, f.t);
  hipLaunchKernelGGL(fetch_fill_kernel, dim3((a.n + kFetchChunk - 1) / kFetchChunk), dim3(kFetchChunk), 0, s, f);
  FetchArgs g = a;  // the gather places from the sums the fill kernel wrote
  g.csum = f.csum_out;
  hipLaunchKernelGGL(fetch_gather_kernel<false>, dim3((a.n + kGR - 1) / kGR), dim3(64 * kFW), 0, s, g);
}

void launch_fetch(const FetchArgs& a, hipStream_t s, const hipEvent_t* ev) {
  if (!a.n) return;
  FetchBatch b{};
  b.nt = 1;
  b.t[0] = a;
  b.rwg0[1] = (a.n + kRW * kRPW - 1) / (kRW * kRPW);
  b.gwg0[1] = (a.n + kGR - 1) / kGR;
  launch_batch(b, s, ev);
}

}  // namespace rmq
