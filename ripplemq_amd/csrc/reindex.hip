// reindex.hip — rebuilding damaged sparse-index entries from the log (rmq_reindex, FORMAT.md §10
// "Index rebuild"), gfx950.
//
// The first pass is the repair's (scrub_common.hpp, launch_repair_scan): one verdict byte per
// (local slot, segment). Three kernels follow on the same plan.
//  * gaps: a lane per segment. A segment that passes on no local slot is bad; a bad segment whose
//    predecessor is not bad heads a gap and is appended to the gap list (one atomic add per wave).
//    RMQ_REINDEX_ALL needs no list: gap g is partition g of the range, its whole log.
//  * walk: a wave per gap, the waves striding over the list. The wave walks the records from the
//    gap's start boundary, finds the record starts from the length words (windows of 64 pieces,
//    the next one in flight), checks up to 64 records at a time, a lane each (records over
//    kBigScrub pieces by the whole wave), on the lowest local slot that passes, and writes the
//    entry of every interval multiple it crosses to a scratch array. Whether the gap resolved
//    goes into the gap's list words.
//  * install: a separate launch, so that the scratch entries and the verdicts of every walk are
//    complete and visible before an index word changes, and so that a lane takes one entry
//    whatever lane of the walk produced it. A wave per resolved gap compares scratch with the
//    stored entries, writes the ones that differ (unless the call is a dry run), counts them and
//    empties the partition's position-cache rows.
//
// Bounds: every ring read is masked with S_p - 1 of the partition's ring. A walk covers
// [pos, lim): pos is the partition's log start or a stored entry, lim its log end or a stored
// entry, and both are used only after the containment checks log_start_pos <= pos <= lim <=
// log_end_pos, 16-byte aligned, of a sane log (no longer than its ring). A length window is read
// only at positions below lim; a record's piece count is clamped by the pieces left before lim
// before a payload piece is loaded. Every record is at least 16 bytes and a position is retried on
// each local slot once, so the iterations are bounded by the span times the slots. An entry index j
// = m - lo comes from positions already checked <= lim <= log_end_pos and is clamped to the gap's
// [s_a, jend) with jend <= nseg - 1, hence m <= hi; the scratch index tbase[i] + j lies inside the
// partition's task range (it has a local slot, so at least nseg tasks) and is checked against the
// array's capacity. A gap list index is checked against the list's capacity. No header word or
// stored entry becomes an address or a loop bound without these.
#include "scrub_common.hpp"

namespace rmq {
namespace {

constexpr u64 kGapSeg = (1ull << 48) - 1ull;  // gap word 0: partition of the range << 48 | first segment
constexpr u64 kGapResolved = 1ull << 63;      // gap word 1: resolved flag | end of the rebuilt entries (jend)
constexpr u64 kGapNone = ~0ull;               // gap word 0 (ALL mode): the partition has no local slot

__device__ __forceinline__ u64* index_slot(const DevState& st, const RingRef& rg, u64 m) {
  return st.index + (rg.ibase + m % rg.icap) * 2;
}

// Segment s of a partition (task base tb, nseg segments on each of its nloc local slots) passes on
// no local slot.
__device__ __forceinline__ bool seg_bad(const uint8_t* verdict, u64 tb, u64 nseg, u32 nloc, u64 s) {
  for (u32 k = 0; k < nloc; ++k)
    if (verdict[tb + (u64)k * nseg + s] == kVerdictPass) return false;
  return true;
}

__device__ __forceinline__ u32 wave_of_grid() {
  return (u32)__builtin_amdgcn_readfirstlane(blockIdx.x * kSW + (threadIdx.x >> 6));
}

// The length words of the 64 pieces of window k (logical positions 1024 k + 16 lane) below lim.
__device__ __forceinline__ u32 ring_lens(const uint8_t* ring, u64 rmask, u64 k, u64 lim, u32 lane) {
  const u64 p = (k << 10) + 16ull * lane;
  return p < lim ? *reinterpret_cast<const u32*>(ring + (p & rmask) + 8ull) : 0u;
}

// What a walk knows of its gap's entries: j = m - lo in [sa, jend) are rebuilt into scratch, and
// (unless the gap ends the log) j == jend is compared with the stored entry {bo, bp}.
struct GapEntries {
  u64* scratch;
  u64 cap, tb, lo, sa, jend, bo, bp;
  u32 ilog;
  bool last;
};
// A record start {o, p}: the entries j in [jl, jh) by steps of `step` (the caller's lanes share a
// range or own one each). Returns 1 if the gap's end entry was met, 3 if it also equals the stored one.
__device__ __forceinline__ u32 assign_entries(const GapEntries& E, u64 o, u64 p, u64 jl, u64 jh, u64 step) {
  const u64 jcap = E.last ? E.jend : E.jend + 1ull;
  if (jl < E.sa) jl = E.sa;
  if (jh > jcap) jh = jcap;
  u32 r = 0;
  for (u64 j = jl; j < jh; j += step) {
    if (j < E.jend) {
      const u64 idx = E.tb + j;
      if (idx < E.cap) *reinterpret_cast<ulonglong2*>(E.scratch + 2ull * idx) = make_ulonglong2(o, p);
    } else {
      r = o == E.bo && p == E.bp ? 3u : 1u;
    }
  }
  return r;
}

}  // namespace

// The verify grid again: a lane per task, of which the first nseg of a partition stand for its
// segments. counts: [n][3] {live entries, entries rewritten, gaps unresolved}.
__global__ __launch_bounds__(kST) void reindex_gaps_kernel(ReindexArgs R) {
  const ScrubArgs& A = R.s;
  const u32 lane = threadIdx.x & 63u;
  const u64 T = A.tbase[A.n];
  const u64 stride = 64ull * gridDim.x * kSW;
  for (u64 t0 = 64ull * wave_of_grid(); t0 < T; t0 += stride) {
    const u64 t = t0 + lane;
    bool head = false;
    u64 word = 0;
    if (t < T) {
      u32 a = 0, b = A.n;
      while (b - a > 1u) {
        const u32 mid = a + ((b - a) >> 1);
        if (A.tbase[mid] <= t) a = mid; else b = mid;
      }
      const u64 tb = A.tbase[a], s = t - tb;
      const ScrubPart q = scrub_part(A.st, A.first + a);
      if (s < q.nseg) {
        const u32 nloc = (u32)__popc(q.mask);
        if (s == 0ull) R.counts[3ull * a] = q.sane && q.nseg > 1ull ? q.nseg - 1ull : 0ull;
        head = seg_bad(R.verdict, tb, q.nseg, nloc, s) && (s == 0ull || !seg_bad(R.verdict, tb, q.nseg, nloc, s - 1ull));
        word = ((u64)a << 48) | (s & kGapSeg);
      }
    }
    const u64 hm = __ballot(head);
    if (hm) {  // (uniform) one add for the wave's heads
      const u32 leader = (u32)__builtin_ctzll(hm);
      u32 base = 0;
      if (lane == leader) base = atomicAdd(R.ngaps, (u32)__popcll(hm));
      base = (u32)__builtin_amdgcn_readlane((int)base, (int)leader);
      if (head) {
        const u64 idx = (u64)base + (u64)__popcll(hm & ((1ull << lane) - 1ull));
        if (idx < R.cap) *reinterpret_cast<ulonglong2*>(R.gaps + 2ull * idx) = make_ulonglong2(word, 0ull);
      }
    }
  }
}

__global__ __launch_bounds__(kST, 4) void reindex_walk_kernel(ReindexArgs R) {
  __shared__ __attribute__((aligned(16))) u32 tabs[16 * 256];  // table[8] then zshift[2][4]
  __shared__ __attribute__((aligned(16))) u32 nibs[512];
  const ScrubArgs& A = R.s;
  crc_tables_lds<kST>(A.crc, tabs, nibs);
  __syncthreads();
  const u32(*t8)[256] = reinterpret_cast<const u32(*)[256]>(tabs);
  const DevState& st = A.st;
  const u32 lane = threadIdx.x & 63u;
  const u32 ilog = st.interval_log2;
  u64 G = A.n;
  if (!R.all) {
    G = *R.ngaps;
    if (G > R.cap) G = R.cap;
  }
  const u64 gstride = (u64)gridDim.x * kSW;
  for (u64 g = wave_of_grid(); g < G; g += gstride) {
    u32 i = (u32)g;
    u64 sa = 0;
    if (!R.all) {
      const u64 w = R.gaps[2ull * g];
      i = (u32)(w >> 48), sa = w & kGapSeg;
    }
    if (i >= A.n) continue;  // (the list holds what the gaps kernel wrote)
    const ScrubPart q = scrub_part(st, A.first + i);
    const u32 nloc = (u32)__popc(q.mask);
    if (R.all) {
      if (!nloc) {
        if (lane == 0u) *reinterpret_cast<ulonglong2*>(R.gaps + 2ull * g) = make_ulonglong2(kGapNone, 0ull);
        continue;
      }
      if (lane == 0u) R.counts[3ull * i] = q.sane && q.nseg > 1ull ? q.nseg - 1ull : 0ull;
    }
    const u64 tb = A.tbase[i];
    bool ok = q.sane && sa < q.nseg && nloc != 0u;
    // the gap's last segment: the one before the first segment after s_a that is not bad
    u64 sb = q.nseg - 1ull;
    if (!R.all && ok) {
      for (u64 s0 = sa + 1ull;; s0 += 64ull) {
        const u64 s = s0 + lane;
        const u64 sm = __ballot(s >= q.nseg || !seg_bad(R.verdict, tb, q.nseg, nloc, s));
        if (sm) {
          sb = s0 + (u64)__builtin_ctzll(sm) - 1ull;
          break;
        }
      }
    }
    GapEntries E;
    E.scratch = R.scratch, E.cap = R.cap, E.tb = tb, E.lo = q.lo, E.sa = sa, E.ilog = ilog;
    E.last = sb + 1ull >= q.nseg;
    E.jend = E.last ? q.nseg - 1ull : sb;
    E.bo = E.bp = 0;
    // the walk's span [pos, lim) and the offset of its first record
    u64 pos = q.sp, expect = q.so, lim = q.ep;
    if (ok && sa > 0ull) {
      const u64* ie = index_slot(st, q.rg, q.lo + sa - 1ull);
      expect = ie[0], pos = ie[1];
    }
    if (ok && !E.last) {
      const u64* ie = index_slot(st, q.rg, q.lo + sb);
      E.bo = ie[0], E.bp = ie[1];
      lim = E.bp;
    }
    ok = ok && q.sp <= pos && pos <= lim && lim <= q.ep && ((pos | lim) & 15ull) == 0ull && q.so <= expect && expect <= q.eo;
    pos = bcast_u64(pos, 0), expect = bcast_u64(expect, 0), lim = bcast_u64(lim, 0);
    const u64 rmask = q.rg.seg - 1ull;
    u32 met = 0;  // assign_entries' result once the gap's end entry is met
    // the starting point is a record start
    if (ok) met = assign_entries(E, expect, pos, E.sa + lane, (pos >> ilog) + 1ull - q.lo, 64ull);
    met = __any(met & 2u) ? 3u : __any(met) ? 1u : 0u;
    u32 rest = q.mask;  // the local slots not yet tried at pos, lowest first
    const uint8_t* ring = st.logs + (u64)(u32)__builtin_ctz(rest) * st.rstride + q.rg.base;
    u64 wk = ~0ull;     // the window in W0 (W1: the one after it)
    u32 W0 = 0, W1 = 0;
    bool dead = false;
    while (ok && !met && !dead && pos < lim) {
      // the next (at most 64) record starts on this slot: lane j keeps the start of record j
      u64 qp = pos, myq = 0;
      u32 nrec = 0;
      while (nrec < 64u && qp < lim) {
        const u64 k = qp >> 10;
        if (k != wk) {
          W0 = wk != ~0ull && k == wk + 1ull ? W1 : ring_lens(ring, rmask, k, lim, lane);
          W1 = ring_lens(ring, rmask, k + 1ull, lim, lane);
          wk = k;
        }
        const u32 Lq = (u32)__builtin_amdgcn_readlane((int)W0, (int)__builtin_amdgcn_readfirstlane((u32)(qp >> 4) & 63u));
        if (lane == nrec) myq = qp;
        qp += 16ull * (1ull + (Lq >> 4) + ((Lq & 15u) ? 1u : 0u));
        ++nrec;
      }
      const bool in = lane < nrec;
      uint4 hdr = make_uint4(0, 0, 0, 0);
      u32 L = 0, m = 0;
      bool chk = false;
      if (in) {  // (myq < lim)
        hdr = load_payload16(ring + (myq & rmask));
        const u64 off = ((u64)hdr.y << 32) | hdr.x;
        L = hdr.z;
        m = (L >> 4) + ((L & 15u) ? 1u : 0u);
        const u64 avail = ((lim - myq) >> 4) - 1ull;  // pieces of the span after this header
        chk = off == expect + lane && (u64)m <= avail;
      }
      bool fail = in && !chk;
      const bool big = chk && m > kBigScrub;
      const u32 mm = chk && !big ? m : 0u;
      const u64 pay = myq + 16ull;
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
      // large records, one at a time by the wave
      for (u64 bm = __ballot(big); bm; bm &= bm - 1ull) {
        const u32 sl = (u32)__builtin_ctzll(bm);
        const u64 bpay = bcast_u64(pay, sl);
        const u32 bm16 = (u32)__builtin_amdgcn_readlane((int)m, (int)sl);  // (at most the span's pieces)
        const u32 bacc = wave_crc_pieces(A.crc, t8, bm16,
                                         [&](u32 jp) { return load_payload16(ring + ((bpay + 16ull * jp) & rmask)); });
        if (lane == sl) acc = bacc;
      }
      if (chk) {
        if (big) padz = pad_zero16(load_payload16(ring + ((myq + 16ull * m) & rmask)), L);
        fail = crc_of_padded(A.crc, acc, L, m) != hdr.w || !padz;
      }
      // the records before the first failing one are accepted; on a slot other than the lowest only
      // the first, so that every position is tried on the lowest slot first
      const u64 fm = __ballot(fail);
      u32 nok = fm ? (u32)__builtin_ctzll(fm) : nrec;
      if (rest != q.mask && nok > 1u) nok = 1u;
      // the start after lane j's record
      u64 ne = ((u64)(u32)__shfl_down((int)(u32)(myq >> 32), 1) << 32) | (u32)__shfl_down((int)(u32)myq, 1);
      if (lane + 1u >= nrec) ne = qp;
      u32 r = 0;
      if (lane < nok) r = assign_entries(E, expect + lane + 1ull, ne, (myq >> ilog) + 1ull - q.lo, (ne >> ilog) + 1ull - q.lo, 1ull);
      met = __any(r & 2u) ? 3u : __any(r) ? 1u : 0u;
      u32 slot = 0;
      bool move = false;
      if (nok) {
        pos = nok == nrec ? qp : bcast_u64(myq, nok);
        expect += nok;
        move = rest != q.mask;
        rest = q.mask;
      } else {
        rest &= rest - 1u;
        dead = rest == 0u;
        move = !dead;
      }
      if (move) {
        slot = (u32)__builtin_ctz(rest);
        ring = st.logs + (u64)slot * st.rstride + q.rg.base;
        wk = ~0ull;
      }
    }
    const bool resolved = ok && !dead && (E.last ? pos == q.ep && expect == q.eo : met == 3u);
    if (lane == 0u) {
      *reinterpret_cast<ulonglong2*>(R.gaps + 2ull * g) =
          make_ulonglong2(((u64)i << 48) | sa, (resolved ? kGapResolved : 0ull) | E.jend);
      if (!resolved) atomicAdd(reinterpret_cast<unsigned long long*>(R.counts + 3ull * i + 2), 1ull);
    }
  }
}

__global__ __launch_bounds__(kST) void reindex_install_kernel(ReindexArgs R) {
  const ScrubArgs& A = R.s;
  const DevState& st = A.st;
  const u32 lane = threadIdx.x & 63u;
  u64 G = A.n;
  if (!R.all) {
    G = *R.ngaps;
    if (G > R.cap) G = R.cap;
  }
  const u64 gstride = (u64)gridDim.x * kSW;
  for (u64 g = wave_of_grid(); g < G; g += gstride) {
    const u64 w0 = R.gaps[2ull * g], w1 = R.gaps[2ull * g + 1ull];
    if (w0 == kGapNone || !(w1 & kGapResolved)) continue;
    const u32 i = (u32)(w0 >> 48);
    if (i >= A.n) continue;
    const u64 sa = w0 & kGapSeg;
    const ScrubPart q = scrub_part(st, A.first + i);
    u64 jend = w1 & ~kGapResolved;
    if (jend > q.nseg - 1ull) jend = q.nseg - 1ull;
    const u64 tb = A.tbase[i];
    u32 cnt = 0;
    for (u64 j = sa + lane; j < jend; j += 64ull) {
      const u64 idx = tb + j;
      if (idx >= R.cap) continue;
      u64* ie = index_slot(st, q.rg, q.lo + j);
      const ulonglong2 nv = *reinterpret_cast<const ulonglong2*>(R.scratch + 2ull * idx);
      if (ie[0] != nv.x || ie[1] != nv.y) {
        ++cnt;
        if (R.write) *reinterpret_cast<ulonglong2*>(ie) = nv;
      }
    }
    const u32 total = (u32)__builtin_amdgcn_readlane((int)wave_incl_scan(cnt), 63);
    if (total) {
      if (lane == 0u) atomicAdd(reinterpret_cast<unsigned long long*>(R.counts + 3ull * i + 1), (unsigned long long)total);
      // a fetch that resolved through a rewritten entry may have cached a position derived from it
      if (R.write)
        for (u32 c = lane; c < st.C; c += 64u)
          *reinterpret_cast<ulonglong2*>(st.pcache + ((u64)(A.first + i) * st.C + c) * 2) = make_ulonglong2(~0ull, 0ull);
    }
  }
}

void launch_reindex(const ReindexArgs& a, uint32_t wgs, hipStream_t s) {
  if (!a.all) hipLaunchKernelGGL(reindex_gaps_kernel, dim3(wgs), dim3(kST), 0, s, a);
  hipLaunchKernelGGL(reindex_walk_kernel, dim3(wgs), dim3(kST), 0, s, a);
  hipLaunchKernelGGL(reindex_install_kernel, dim3(wgs), dim3(kST), 0, s, a);
}

}  // namespace rmq
