// scrub_common.hpp — what the scrub (scrub.hip) and the repair (repair.hip) share: a partition's
// segments, the task -> (partition, local slot, segment) decoding with its containment checks, and
// the verify walk (FORMAT.md §10).
//
// Bounds: every ring read is masked with S_p - 1 of that partition's ring (ring_ref), a record's
// piece count is clamped by the pieces left in its segment before any payload piece is loaded, a
// segment is accepted only inside [log_start_pos, log_end_pos) of a log no longer than its ring,
// and a walk ends at its segment's end: every record is at least 16 bytes, so the iterations are
// bounded by the segment's span. No header word is an address or a loop bound without these.
#pragma once
#include "device_common.hpp"
#include "kernels.hpp"

namespace rmq {

constexpr u32 kST = 256;        // threads per verify workgroup
constexpr u32 kSW = kST / 64;   // its waves
constexpr u32 kBigScrub = 64;   // records over this many 16-byte pieces: the whole wave (kBigIngest)

// What the plan and the verify lanes both derive of partition p: its retained log, its ring, its
// local replica slots and the segments that tile the log (FORMAT.md §10).
struct ScrubPart {
  u64 so, sp, eo, ep;  // log start / end {offset, position}
  u64 lo;              // first live index entry, ceil(sp / I)
  u64 nseg;            // segments: 1 (no live entry, or a state no log can have), else hi - lo + 2
  RingRef rg;
  u32 mask;            // local replica slots
  bool sane;           // the log lies forward, 16-byte aligned, inside one ring length
};
__device__ __forceinline__ ScrubPart scrub_part(const DevState& st, u32 p) {
  ScrubPart q;
  q.so = st.start_off[p];
  q.sp = st.start_pos[p];
  q.eo = st.leo[p];
  q.ep = st.used[p];
  q.rg = ring_ref(st, p);
  q.mask = st.local_mask[p] & ((1u << st.RF) - 1u);
  q.sane = q.ep >= q.sp && q.ep - q.sp <= q.rg.seg && ((q.sp | q.ep) & 15ull) == 0ull && q.eo >= q.so;
  const u32 ilog = st.interval_log2;
  q.lo = (q.sp + (1ull << ilog) - 1ull) >> ilog;
  const u64 hi = q.ep >> ilog;
  q.nseg = q.sane && q.lo <= hi ? hi - q.lo + 2ull : 1ull;
  return q;
}

__device__ __forceinline__ u64 scrub_key(u64 off, u32 replica, u32 kind) {
  return (off << 5) | ((u64)replica << 2) | kind;
}

// Task t of a plan: partition first + i, local replica slot r (the ri-th set bit of its mask),
// segment s of nseg: bytes [pos, end), offsets [expect, eoff). kind != 0: the segment failed the
// containment checks (pos = end = 0: it has no bounds).
struct ScrubTask {
  u32 i, r, kind, mask;
  u64 ri, s, nseg;
  u64 pos, end, expect, eoff, rmask, bad_off;
  const uint8_t* ring;
};
__device__ __forceinline__ ScrubTask scrub_task(const ScrubArgs& A, u64 t) {
  const DevState& st = A.st;
  ScrubTask k;
  // the partition whose task range holds t: the largest i with tbase[i] <= t
  u32 a = 0, b = A.n;
  while (b - a > 1u) {
    const u32 mid = a + ((b - a) >> 1);
    if (A.tbase[mid] <= t) a = mid; else b = mid;
  }
  k.i = a;
  const ScrubPart q = scrub_part(st, A.first + k.i);
  const u64 tl = t - A.tbase[k.i];
  k.nseg = q.nseg;
  k.mask = q.mask;
  k.ri = tl / q.nseg, k.s = tl - k.ri * q.nseg;
  u32 mk = q.mask;
  for (u64 j = 0; j < k.ri && mk; ++j) mk &= mk - 1u;  // (ri < popc(mask): the plan's count)
  k.r = mk ? (u32)__builtin_ctz(mk) : 0u;
  k.rmask = q.rg.seg - 1ull;
  k.ring = st.logs + (u64)k.r * st.rstride + q.rg.base;
  k.kind = 0, k.bad_off = 0;
  k.pos = k.end = k.expect = k.eoff = 0;
  if (!q.sane) {
    k.kind = kScrubBadChain;
    k.bad_off = q.so;
  } else {
    k.pos = q.sp, k.expect = q.so, k.end = q.ep, k.eoff = q.eo;
    if (q.nseg > 1ull) {
      if (k.s > 0ull) {
        const u64* ie = st.index + (q.rg.ibase + (q.lo + k.s - 1ull) % q.rg.icap) * 2;
        k.expect = ie[0], k.pos = ie[1];
      }
      if (k.s + 1ull < q.nseg) {
        const u64* ie = st.index + (q.rg.ibase + (q.lo + k.s) % q.rg.icap) * 2;
        k.eoff = ie[0], k.end = ie[1];
      }
    }
    // the entries name positions and offsets inside the log, in order
    if (!(q.sp <= k.pos && k.pos <= k.end && k.end <= q.ep && ((k.pos | k.end) & 15ull) == 0ull && q.so <= k.expect &&
          k.expect <= k.eoff && k.eoff <= q.eo)) {
      k.kind = kScrubBadChain;
      k.bad_off = k.expect < q.so ? q.so : k.expect > q.eo ? q.eo : k.expect;
      k.pos = k.end = 0;
    }
  }
  return k;
}

// Verdict bytes of the repair's first pass, one per task (a lane's own byte: no two lanes share a
// store).
constexpr uint8_t kVerdictPass = 1, kVerdictFail = 2;

// The verify walk of a workgroup of kST threads: its waves take blocks of 64 tasks w, w + waves,
// ..., one lane per segment. kVerdict: additionally store each task's verdict at verdict[t].
// tabs: 16 KB of LDS for table[8] then zshift[2][4]; nibs: 2 KB of scratch.
template <bool kVerdict>
__device__ __forceinline__ void scrub_verify_body(const ScrubArgs& A, uint8_t* verdict, u32* tabs, u32* nibs) {
  crc_tables_lds<kST>(A.crc, tabs, nibs);
  __syncthreads();
  const u32(*t8)[256] = reinterpret_cast<const u32(*)[256]>(tabs);
  const DevState& st = A.st;
  const u32 lane = threadIdx.x & 63u;
  const u64 T = A.tbase[A.n];
  const u64 stride = 64ull * gridDim.x * kSW;
  for (u64 t0 = 64ull * (u32)__builtin_amdgcn_readfirstlane(blockIdx.x * kSW + (threadIdx.x >> 6)); t0 < T; t0 += stride) {
    const u64 t = t0 + lane;
    const bool in = t < T;
    u32 i = ~0u, r = 0;
    // the segment: bytes [pos, end), offsets [expect, eoff)
    u64 pos = 0, end = 0, expect = 0, eoff = 0, rmask = 0;
    const uint8_t* ring = st.logs;
    u32 kind = 0;      // RMQ_SCRUB_BAD_* of the lane's failing record
    u64 bad_off = 0;   // its expected offset
    if (in) {
      const ScrubTask k = scrub_task(A, t);
      i = k.i, r = k.r, rmask = k.rmask, ring = k.ring;
      kind = k.kind, bad_off = k.bad_off;
      pos = k.pos, end = k.end, expect = k.expect, eoff = k.eoff;
    }
    u64 n_ok = 0, b_ok = 0;
    bool live = in && !kind && pos < end;
    while (__any(live)) {
      uint4 hdr = make_uint4(0, 0, 0, 0);
      u32 L = 0, m = 0;
      bool chk = false;
      if (live) {
        hdr = load_payload16(ring + (pos & rmask));
        const u64 off = ((u64)hdr.y << 32) | hdr.x;
        L = hdr.z;
        m = (L >> 4) + ((L & 15u) ? 1u : 0u);
        const u64 avail = ((end - pos) >> 4) - 1ull;  // pieces of the segment after this header
        if (off != expect || (u64)m > avail) {  // out of sequence, or the record runs past its segment
          kind = kScrubBadChain;
          bad_off = expect;
          live = false;
        } else {
          chk = true;
        }
      }
      const bool big = chk && m > kBigScrub;
      const u32 mm = chk && !big ? m : 0u;
      const u64 pay = pos + 16ull;
      // the CRC register over the payload pieces in order (zero-padded in the log), from ~0
      u32 acc = 0xFFFFFFFFu;
      bool padz = true;
      for (u32 c = 0; __any(c < mm); c += 4) {
        uint4 v[4];
#pragma unroll
        for (u32 u = 0; u < 4; ++u)  // four pieces in flight per lane
          v[u] = c + u < mm ? load_payload16(ring + ((pay + 16ull * (c + u)) & rmask)) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (u32 u = 0; u < 4; ++u)
          if (c + u < mm) {
            acc = crc_step8(t8, crc_step8(t8, acc, v[u].x, v[u].y), v[u].z, v[u].w);
            if (c + u + 1u == mm) padz = pad_zero16(v[u], L);
          }
      }
      // large records, one at a time by the wave (the 1 KB Horner shift)
      for (u64 bm = __ballot(big); bm; bm &= bm - 1ull) {
        const u32 sl = (u32)__builtin_ctzll(bm);
        const uint8_t* bring = reinterpret_cast<const uint8_t*>(bcast_u64(reinterpret_cast<u64>(ring), sl));
        const u64 bpay = bcast_u64(pay, sl), bmask = bcast_u64(rmask, sl);
        const u32 bm16 = (u32)__builtin_amdgcn_readlane((int)m, (int)sl);  // (at most the segment's pieces)
        const u32 bacc = wave_crc_pieces(A.crc, t8, bm16,
                                         [&](u32 jp) { return load_payload16(bring + ((bpay + 16ull * jp) & bmask)); });
        if (lane == sl) acc = bacc;
      }
      if (chk) {
        const u32 crc = crc_of_padded(A.crc, acc, L, m);
        // (a large record's last piece is read again: the wave folded its pieces)
        if (big) padz = pad_zero16(load_payload16(ring + ((pos + 16ull * m) & rmask)), L);
        if (crc == hdr.w && padz) {
          const u64 rs = 16ull * (1ull + m);
          ++n_ok;
          b_ok += rs;
          pos += rs;
          ++expect;
          live = pos < end;
        } else {
          kind = kScrubBadCrc;
          bad_off = expect;
          live = false;
        }
      }
    }
    // the walk landed on the segment's end (a record never passes it): as many records as the
    // index says
    if (in && !kind && expect != eoff) {
      kind = kScrubBadChain;
      bad_off = expect < eoff ? expect : eoff;
    }
    if constexpr (kVerdict) if (in) verdict[t] = kind ? kVerdictFail : kVerdictPass;
    if (in && kind) atomicMin(reinterpret_cast<unsigned long long*>(A.rows + 4ull * i), (unsigned long long)scrub_key(bad_off, r, kind));
    // records and bytes that passed: one add per run of a partition's lanes in the wave
    const u32 prev = (u32)__shfl_up((int)i, 1), next = (u32)__shfl_down((int)i, 1);
    const u32 head = lane == 0u || prev != i ? 1u : 0u;
    const bool tail = lane == 63u || next != i;
    u32 f1 = head, f2 = head;
    wave_seg_incl_scan(f1, n_ok);
    wave_seg_incl_scan(f2, b_ok);
    if (in && tail && n_ok) {
      atomicAdd(reinterpret_cast<unsigned long long*>(A.rows + 4ull * i + 1), (unsigned long long)n_ok);
      atomicAdd(reinterpret_cast<unsigned long long*>(A.rows + 4ull * i + 2), (unsigned long long)b_ok);
    }
  }
}

}  // namespace rmq
