// restore.hip — loading replica logs from record images (rmq_restore, FORMAT.md §11), gfx950.
//
// The host hands over runs of FORMAT.md §1 records with the position of every record (what
// rmq_scan_records / rmq_tier_append wrote when the files were made), so both passes take a lane per
// record, 64 records per wave, as the follower's ingest_verify_kernel does:
//   verify   every record of every item against the §11 rules; a failure lowers the item's key
//            (expected offset << 5 | kind) with one 64-bit atomicMin, as the scrub's rows do;
//   install  only items whose key is still clean: the record's 16-byte pieces into the ring of every
//            local replica slot at pos mod S_p, and the sparse-index entries the record writes (§5);
//            a wave whose 64 records are one item's copies their contiguous span as one;
//   finish   a thread per item: the partition's state, E[first_pos / I], the position cache.
// The three launches follow each other on the pipeline stream: no byte is written before every
// verdict of the call is in.
//
// Bounds. The host checked every item: the run [run, run + bytes) and the count + 1 table words lie
// inside the device buffers, bytes <= S_p, everything a multiple of 16, count <= bytes / 16. On the
// device a record's two table words (t0, t1) are used only once t0 < t1 <= bytes, both multiples of
// 16 (tab_ok): then the header at run + t0 and the (t1 - t0) / 16 - 1 payload pieces behind it lie
// inside the run. The length word is never an address or a loop bound: 16 + align16(len) must EQUAL
// t1 - t0 before any payload piece is loaded, and the piece count is derived from t1 - t0. Ring
// stores are masked with S_p - 1 of the partition's own ring; index slots are taken modulo the
// partition's own index ring, which holds more entries than a window of S_p bytes crosses intervals.
#include "scrub_common.hpp"

namespace rmq {
namespace {

// Record g of the call: item j, record k of it, its table words, and whether they may be used.
struct RestoreRec {
  u32 j;
  u64 k, t0, t1;
  bool tab_ok;
};
__device__ __forceinline__ RestoreRec restore_rec(const RestoreArgs& A, u64 g) {
  RestoreRec r;
  // the item whose record range holds g: the largest j with rbase[j] <= g (empty items share a base
  // with the next one and are passed over)
  u32 a = 0, b = A.n;
  while (b - a > 1u) {
    const u32 mid = a + ((b - a) >> 1);
    if (A.rbase[mid] <= g) a = mid; else b = mid;
  }
  r.j = a;
  r.k = g - A.rbase[a];
  const RestoreItem& it = A.items[a];
  r.t0 = it.tab[r.k];
  r.t1 = it.tab[r.k + 1ull];
  r.tab_ok = ((r.t0 | r.t1) & 15ull) == 0ull && r.t0 < r.t1 && r.t1 <= it.bytes && (r.k != 0ull || r.t0 == 0ull) &&
             (r.k + 1ull != it.count || r.t1 == it.bytes);
  return r;
}

__device__ __forceinline__ u32 uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }

// waves stride over blocks of 64 records
__device__ __forceinline__ u64 first_block() {
  return 64ull * (u32)__builtin_amdgcn_readfirstlane(blockIdx.x * kSW + (threadIdx.x >> 6));
}

}  // namespace

__global__ __launch_bounds__(kST) void restore_verify_kernel(RestoreArgs A) {
  __shared__ __attribute__((aligned(16))) u32 tabs[16 * 256];  // table[8] then zshift[2][4]
  __shared__ __attribute__((aligned(16))) u32 nibs[512];
  crc_tables_lds<kST>(A.crc, tabs, nibs);
  __syncthreads();
  const u32(*t8)[256] = reinterpret_cast<const u32(*)[256]>(tabs);
  const u32 lane = threadIdx.x & 63u;
  const u64 R = A.rbase[A.n];
  const u64 stride = 64ull * gridDim.x * kSW;
  for (u64 g0 = first_block(); g0 < R; g0 += stride) {
    const u64 g = g0 + lane;
    const bool in = g < R;
    u32 j = 0, kind = 0, L = 0, m = 0;
    u64 expect = 0;
    const uint8_t* rec = nullptr;
    uint4 hdr = make_uint4(0, 0, 0, 0);
    bool chk = false;
    if (in) {
      const RestoreRec r = restore_rec(A, g);
      const RestoreItem& it = A.items[r.j];
      j = r.j;
      expect = it.first_off + r.k;
      kind = kScrubBadChain;  // until the table, the offset and the extent hold
      if (r.tab_ok) {
        rec = it.run + r.t0;
        hdr = *reinterpret_cast<const uint4*>(rec);
        const u64 off = ((u64)hdr.y << 32) | hdr.x;
        L = hdr.z;
        const u64 m64 = (u64)(L >> 4) + ((L & 15u) ? 1ull : 0ull);
        if (off == expect && 16ull * (1ull + m64) == r.t1 - r.t0) {
          m = (u32)m64;  // (the pieces between the two table words: inside the run)
          chk = true;
          kind = 0;
        }
      }
    }
    const bool big = chk && m > kBigScrub;
    const u32 mm = chk && !big ? m : 0u;
    // the CRC register over the payload pieces in order (zero-padded in the image), from ~0
    u32 acc = 0xFFFFFFFFu;
    bool padz = true;
    for (u32 c = 0; __any(c < mm); c += 4) {
      uint4 v[4];
#pragma unroll
      for (u32 u = 0; u < 4; ++u)  // four pieces in flight per lane
        v[u] = c + u < mm ? *reinterpret_cast<const uint4*>(rec + 16ull * (1ull + c + u)) : make_uint4(0, 0, 0, 0);
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
      const uint8_t* brec = reinterpret_cast<const uint8_t*>(bcast_u64(reinterpret_cast<u64>(rec), sl));
      const u32 bm16 = (u32)__builtin_amdgcn_readlane((int)m, (int)sl);
      const u32 bacc = wave_crc_pieces(A.crc, t8, bm16, [&](u32 jp) {
        return *reinterpret_cast<const uint4*>(brec + 16ull * (1ull + jp));
      });
      if (lane == sl) acc = bacc;
    }
    if (chk) {
      // (a large record's last piece is read again: the wave folded its pieces)
      if (big) padz = pad_zero16(*reinterpret_cast<const uint4*>(rec + 16ull * m), L);
      if (crc_of_padded(A.crc, acc, L, m) != hdr.w || !padz) kind = kScrubBadCrc;
    }
    if (in && kind) atomicMin(reinterpret_cast<unsigned long long*>(A.key + j), (unsigned long long)scrub_key(expect, 0u, kind));
  }
}

// Records of the items that passed, into the rings and the index. Nothing reads the rings back in
// this call, so the stores are the log's non-temporal 16-byte stores.
__global__ __launch_bounds__(kST) void restore_install_kernel(RestoreArgs A) {
  const DevState& st = A.st;
  const u32 lane = threadIdx.x & 63u;
  const u64 R = A.rbase[A.n];
  const u64 stride = 64ull * gridDim.x * kSW;
  for (u64 g0 = first_block(); g0 < R; g0 += stride) {
    const u64 g = g0 + lane;
    const uint8_t* rec = nullptr;
    uint8_t* ring = nullptr;  // the partition's ring in replica region 0
    u64 pos = 0, rmask = 0;
    u32 np = 0, slots = 0;    // 16-byte pieces of the record, header included; local slots
    u32 jl = ~0u;             // its item
    if (g < R) {
      const RestoreRec r = restore_rec(A, g);
      const RestoreItem& it = A.items[r.j];
      if (A.key[r.j] == kScrubClean && r.tab_ok) {  // (clean: every record's table words passed)
        jl = r.j;
        const RingRef rg = ring_ref(st, it.pidx);
        rec = it.run + r.t0;
        np = (u32)((r.t1 - r.t0) >> 4);
        pos = it.first_pos + r.t0;
        rmask = rg.seg - 1ull;
        ring = st.logs + rg.base;
        slots = st.local_mask[it.pidx] & ((1u << st.RF) - 1u);
        // sparse index: every interval multiple the record crosses names the next record (§5)
        const u32 ilog = st.interval_log2;
        const u64 end = it.first_pos + r.t1;
        for (u64 q = (pos >> ilog) + 1ull; (q << ilog) <= end; ++q) {
          u64* ie = st.index + (rg.ibase + q % rg.icap) * 2;
          ie[0] = it.first_off + r.k + 1ull;
          ie[1] = end;
        }
      }
    }
    // 64 records of ONE item: lane l's second table word is lane l + 1's first, so they are one
    // contiguous span of the run (at most the item's bytes, hence at most S_p), which the wave copies
    // as one, 64 lanes x 16 bytes a step: every store instruction covers 1 KB of a ring, where a
    // lane per record stores 16 bytes a record size apart
    if (__all(jl != ~0u && jl == uni(jl))) {
      const uint8_t* brec = reinterpret_cast<const uint8_t*>(bcast_u64(reinterpret_cast<u64>(rec), 0u));
      uint8_t* bring = reinterpret_cast<uint8_t*>(bcast_u64(reinterpret_cast<u64>(ring), 0u));
      const u64 bpos = bcast_u64(pos, 0u), bmask = bcast_u64(rmask, 0u);
      const u64 len = bcast_u64(pos + 16ull * np, 63u) - bpos;
      const u32 bslots = uni(slots);
      for (u64 o0 = 16ull * lane; o0 < len; o0 += 4096ull) {
        uint4 v[4];
#pragma unroll
        for (u32 u = 0; u < 4; ++u)
          v[u] = o0 + 1024ull * u < len ? load_payload16(brec + o0 + 1024ull * u) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (u32 u = 0; u < 4; ++u)
          if (o0 + 1024ull * u < len)
            for (u32 mk = bslots; mk; mk &= mk - 1u)
              store_log16(bring + (u64)__builtin_ctz(mk) * st.rstride + ((bpos + o0 + 1024ull * u) & bmask), v[u]);
      }
      continue;
    }
    // a block that ends an item or the call: a lane per record
    const bool big = np > kBigScrub + 1u;
    const u32 nn = big ? 0u : np;
    for (u32 c = 0; __any(c < nn); c += 4) {
      uint4 v[4];
#pragma unroll
      for (u32 u = 0; u < 4; ++u)
        v[u] = c + u < nn ? load_payload16(rec + 16ull * (c + u)) : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (u32 u = 0; u < 4; ++u)
        if (c + u < nn)
          for (u32 mk = slots; mk; mk &= mk - 1u)
            store_log16(ring + (u64)__builtin_ctz(mk) * st.rstride + ((pos + 16ull * (c + u)) & rmask), v[u]);
    }
    // large records, one at a time by the wave: 64 lanes x 16 bytes per step
    for (u64 bm = __ballot(big); bm; bm &= bm - 1ull) {
      const u32 sl = (u32)__builtin_ctzll(bm);
      const uint8_t* brec = reinterpret_cast<const uint8_t*>(bcast_u64(reinterpret_cast<u64>(rec), sl));
      uint8_t* bring = reinterpret_cast<uint8_t*>(bcast_u64(reinterpret_cast<u64>(ring), sl));
      const u64 bpos = bcast_u64(pos, sl), bmask = bcast_u64(rmask, sl);
      const u32 bnp = (u32)__builtin_amdgcn_readlane((int)np, (int)sl);
      const u32 bslots = (u32)__builtin_amdgcn_readlane((int)slots, (int)sl);
      for (u32 c = lane; c < bnp; c += 64u) {
        const uint4 v = load_payload16(brec + 16ull * c);
        for (u32 mk = bslots; mk; mk &= mk - 1u)
          store_log16(bring + (u64)__builtin_ctz(mk) * st.rstride + ((bpos + 16ull * c) & bmask), v);
      }
    }
  }
}

// The state of every item that passed (a thread per item), after its records are in.
__global__ void restore_finish_kernel(RestoreArgs A) {
  const DevState& st = A.st;
  const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= A.n || A.key[j] != kScrubClean) return;
  const RestoreItem& it = A.items[j];
  const u32 p = it.pidx, ilog = st.interval_log2;
  const u64 leo = it.first_off + it.count, used = it.first_pos + it.bytes;
  if (!(it.first_pos & ((1ull << ilog) - 1ull))) {  // as the follower's rebase does (§9 step 3)
    const RingRef rg = ring_ref(st, p);
    u64* ie = st.index + (rg.ibase + (it.first_pos >> ilog) % rg.icap) * 2;
    ie[0] = it.first_off;
    ie[1] = it.first_pos;
  }
  st.start_off[p] = it.first_off;
  st.start_pos[p] = it.first_pos;
  for (u32 s = 0; s < 2; ++s) {
    A.sets[s].leo[p] = leo;
    A.sets[s].used[p] = used;
  }
  st.commit[p] = st.hw[p] = st.lcommit[p] = it.commit;
  const u32 mask = st.local_mask[p];
  for (u32 r = 0; r < st.RF; ++r) st.match[(u64)p * st.RF + r] = (mask >> r) & 1u ? leo : 0ull;
  for (u32 c = 0; c < st.C; ++c) {
    u64* pc = st.pcache + ((u64)p * st.C + c) * 2;
    pc[0] = ~0ull;
    pc[1] = 0ull;
  }
}

static uint32_t restore_grid(uint64_t records, uint32_t max_wgs) {
  const uint64_t blocks = (records + 63ull) / 64ull;
  const uint64_t wgs = (blocks + kSW - 1) / kSW;
  return (uint32_t)(wgs < max_wgs ? wgs : max_wgs);
}

void launch_restore_verify(const RestoreArgs& a, uint64_t records, uint32_t max_wgs, hipStream_t s) {
  if (records) hipLaunchKernelGGL(restore_verify_kernel, dim3(restore_grid(records, max_wgs)), dim3(kST), 0, s, a);
}

void launch_restore_install(const RestoreArgs& a, uint64_t records, uint32_t max_wgs, hipStream_t s) {
  if (records) hipLaunchKernelGGL(restore_install_kernel, dim3(restore_grid(records, max_wgs)), dim3(kST), 0, s, a);
  if (a.n) hipLaunchKernelGGL(restore_finish_kernel, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace rmq
